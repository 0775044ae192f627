"""DataStats / ReduceDtypeSize / DropLowCardinality / AddMetadata: everything that needs no device
-- the dtype choice, the schema effects, the selector, Workflow.fit's schema refresh, the argument
checks of the two C entry points, graph.json records and the host arithmetic of the statistics."""
import ctypes as C
import json
import math

import numpy as np
import pandas as pd
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import _lib, graph_json, ops
from nvtabular_amd.ops import _profile as P
from nvtabular_amd.schema import ColumnSchema, Schema, Tags


# ---- (min, max) -> dtype ---------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,want", [
    (0, 127, "int8"), (0, 128, "int16"), (-128, 0, "int8"), (-129, 0, "int16"),
    (0, 32767, "int16"), (0, 32768, "int32"), (-32768, 0, "int16"), (-32769, 0, "int32"),
    (0, 2**31 - 1, "int32"), (0, 2**31, "int64"), (-(2**31), 0, "int32"), (-(2**31) - 1, 0, "int64"),
    (-(2**63), 2**63 - 1, "int64"), (5, 5, "int8"), (-128, 127, "int8"), (-129, 127, "int16"),
])
def test_reduced_dtype_integer_boundaries(lo, hi, want):
    assert P.reduced_dtype(np.int64, lo, hi) == np.dtype(want)
    # never wider than the input
    assert P.reduced_dtype(np.int32, lo, hi) == np.dtype(want if np.dtype(want).itemsize < 4 else "int32")


def test_reduced_dtype_floats_empty_and_other_kinds():
    nan = float("nan")
    assert P.reduced_dtype(np.float64, -1.5, 2.5) == np.dtype("float32")
    assert P.reduced_dtype(np.float64, -1.5, 2.5, np.float64) == np.dtype("float64")
    assert P.reduced_dtype(np.float32, 0.0, 1.0) == np.dtype("float32")
    assert P.reduced_dtype(np.float32, 0.0, 1.0, np.float64) == np.dtype("float32")   # never wider than the input
    assert P.reduced_dtype(np.float64, -np.inf, np.inf) == np.dtype("float32")
    for dt in (np.int64, np.int32, np.float64):
        assert P.reduced_dtype(dt, None, None) == np.dtype(dt)        # no valid row
        assert P.reduced_dtype(dt, nan, nan) == np.dtype(dt)
        assert P.reduced_dtype(dt, nan, 3) == np.dtype(dt)
    for dt in (np.uint8, np.bool_, object):
        assert P.reduced_dtype(dt, 0, 1) == np.dtype(dt)              # anything else: unchanged


# ---- AddMetadata -----------------------------------------------------------------------------------
def _schema():
    return Schema([ColumnSchema("u", np.int64, tags=(Tags.CATEGORICAL,), properties={"p": 1}),
                   ColumnSchema("x", np.float32)])


@pytest.mark.parametrize("op,tags,props", [
    (ops.AddMetadata(tags=[Tags.TARGET], properties={"a": 2}), [Tags.TARGET], {"a": 2}),
    (ops.AddMetadata(), [], {}),
    (ops.AddTags([Tags.REGRESSION, Tags.TARGET]), [Tags.REGRESSION, Tags.TARGET], {}),
    (ops.AddProperties({"domain": {"min": 0, "max": 9}}), [], {"domain": {"min": 0, "max": 9}}),
    (ops.TagAsUserID(), [Tags.ID, Tags.USER], {}),
    (ops.TagAsItemID(), [Tags.ID, Tags.ITEM], {}),
    (ops.TagAsUserFeatures(), [Tags.USER], {}),
    (ops.TagAsItemFeatures(), [Tags.ITEM], {}),
], ids=lambda v: type(v).__name__ if isinstance(v, ops.Operator) else "")
def test_add_metadata_schema_effects(op, tags, props):
    wf = nvt.Workflow(["u", "x"] >> op)
    wf.fit_schema(_schema())
    out = wf.output_schema
    assert out.column_names == ["u", "x"]
    assert list(out["u"].tags) == [Tags.CATEGORICAL] + tags and list(out["x"].tags) == tags
    assert out["u"].properties == {"p": 1, **props} and out["x"].properties == props
    assert out["u"].dtype == np.dtype(np.int64) and out["x"].dtype == np.dtype(np.float32)
    df = pd.DataFrame({"u": [1], "x": [2.0]})
    assert op.transform(nvt.ColumnSelector(["u", "x"]), df) is df


# ---- DropLowCardinality ------------------------------------------------------------------------------
def test_drop_low_cardinality_selector():
    cat = (Tags.CATEGORICAL,)
    schema = Schema([
        ColumnSchema("nodomain", np.int64, tags=cat),
        ColumnSchema("below", np.int64, tags=cat, properties={"domain": {"min": 0, "max": 3}}),
        ColumnSchema("equal", np.int64, tags=cat, properties={"domain": {"min": 0, "max": 4}}),
        ColumnSchema("above", np.int64, tags=cat, properties={"domain": {"min": 0, "max": 5}}),
        ColumnSchema("cont", np.float32, tags=(Tags.CONTINUOUS,), properties={"domain": {"min": 0, "max": 1}}),
        ColumnSchema("plain", np.int64),
    ])
    op = ops.DropLowCardinality()
    assert op.selector_from_fit and not ops.Operator.selector_from_fit and not ops.Categorify.selector_from_fit
    sel = op.compute_selector(schema, nvt.ColumnSelector(schema.column_names), None, None)
    assert sel.names == ["cont", "plain", "nodomain", "equal", "above"]
    assert ops.DropLowCardinality(min_cardinality=6).compute_selector(
        schema, nvt.ColumnSelector(schema.column_names)).names == ["cont", "plain", "nodomain"]
    assert ops.DropLowCardinality(min_cardinality=0).compute_selector(
        schema, nvt.ColumnSelector(["below"])).names == ["cont", "plain", "nodomain", "below", "equal", "above"]
    with pytest.raises(ValueError, match="missing"):
        op.compute_selector(schema, nvt.ColumnSelector(["below", "missing"]))
    # through the graph: the output schema drops the column
    wf = nvt.Workflow(schema.column_names >> op)
    wf.fit_schema(schema)
    assert wf.output_schema.column_names == ["cont", "plain", "nodomain", "equal", "above"]


class _CountingWorkflow(nvt.Workflow):
    calls = 0

    def fit_schema(self, schema):
        type(self).calls += 1
        return super().fit_schema(schema)


class _Part(list):
    """Stand-in dataset: a schema and no partitions (nothing reaches a device)."""

    def __init__(self, schema):
        super().__init__()
        self.schema = schema

    def to_iter(self, columns=None, shard=None):
        return iter(())


def test_fit_refreshes_schemas_only_for_selector_from_fit_graphs():
    schema = _schema()

    def calls(graph):
        class W(_CountingWorkflow):
            calls = 0
        wf = W(graph)
        wf.fit(_Part(schema))
        before = W.calls
        stale = wf._stale_schema_root
        _ = wf.output_schema
        return before, W.calls, stale

    # a graph without such an operator: ONE fit_schema in fit (the schemas of a new input), the
    # fitted properties folded in lazily by the first output_schema -- what fit did before
    assert calls(["u", "x"] >> ops.AddTags([Tags.USER])) == (1, 2, schema)
    assert calls(["u", "x"] >> ops.TagAsItemID() >> ops.AddProperties({"k": 1})) == (1, 2, schema)
    # with one (no StatOperator, so no fit phase): nothing is left to refresh lazily
    before, after, stale = calls(["u", "x"] >> ops.DropLowCardinality())
    assert (before, after, stale) == (1, 1, None)


def test_fit_refreshes_behind_every_phase():
    class Stat(ops.StatOperator):
        def fit_begin(self, sel):
            return {}

        def fit_partition(self, state, sel, df):
            pass

        def fit_end(self, state, sel):
            return {}

        def fit_finalize(self, stats):
            pass

        def clear(self):
            pass

    class W(_CountingWorkflow):
        calls = 0

    wf = W(["u", "x"] >> Stat() >> Stat() >> ops.DropLowCardinality())
    wf.fit(_Part(_schema()))
    assert W.calls == 1 + 2 and wf._stale_schema_root is None      # two phases, one refresh each

    class V(_CountingWorkflow):
        calls = 0

    wf = V(["u", "x"] >> Stat() >> Stat())
    wf.fit(_Part(_schema()))
    assert V.calls == 1 and wf._stale_schema_root is not None


# ---- C ABI: refusals that come before any launch -----------------------------------------------------
def _refused(lib, rc, *words):
    assert rc == _lib.NVT_EINVAL, (rc, lib.nvt_last_error())
    msg = lib.nvt_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_col_profile_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)

    def desc(**kw):
        c = dict(x=p, valid=None, n=8, dtype=_lib.NVT_I64, counts=p, extrema=p + 16, sums=p + 32)
        c.update(kw)
        return (_lib.ProfileCol * 1)(_lib.ProfileCol(**c))

    _refused(lib, lib.nvt_col_profile_many(None, 1, p, None), b"null descriptors")
    _refused(lib, lib.nvt_col_profile_many(desc(), 0, p, None), b"ncols")
    _refused(lib, lib.nvt_col_profile_many(desc(), -1, p, None), b"ncols")
    _refused(lib, lib.nvt_col_profile_many(desc(), 1, None, None), b"partials")
    for name in ("counts", "extrema", "sums"):
        _refused(lib, lib.nvt_col_profile_many(desc(**{name: None}), 1, p, None), b"null accumulator")
        _refused(lib, lib.nvt_col_profile_many(desc(n=0, **{name: None}), 1, p, None), b"null accumulator")
    for dt in (_lib.NVT_U8, _lib.NVT_I8, _lib.NVT_I16, 7, -1):
        _refused(lib, lib.nvt_col_profile_many(desc(dtype=dt), 1, p, None), b"unsupported dtype")
    _refused(lib, lib.nvt_col_profile_many(desc(x=None), 1, p, None), b"x must be")
    _refused(lib, lib.nvt_col_profile_many(desc(x=p + 4), 1, p, None), b"aligned to its element size")
    _refused(lib, lib.nvt_col_profile_many(desc(x=p + 2, dtype=_lib.NVT_F32), 1, p, None), b"aligned")
    # a second descriptor is checked before the first is launched
    two = (_lib.ProfileCol * 2)(desc()[0], desc(dtype=9)[0])
    _refused(lib, lib.nvt_col_profile_many(two, 2, p, None), b"unsupported dtype")
    # zero rows: nothing to launch, the accumulators are not touched
    buf[0] = 77
    assert lib.nvt_col_profile_many(desc(n=0, x=None), 1, p, None) == 0 and buf[0] == 77


def test_cast_entry_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    I8, I16, I32, I64, F32, F64, U8 = (_lib.NVT_I8, _lib.NVT_I16, _lib.NVT_I32, _lib.NVT_I64, _lib.NVT_F32,
                                       _lib.NVT_F64, _lib.NVT_U8)

    def desc(src_dtype, dst_dtype, src=p, dst=p + 256, n=8):
        return (_lib.CastCol * 1)(_lib.CastCol(src=src, dst=dst, n=n, src_dtype=src_dtype, dst_dtype=dst_dtype))

    _refused(lib, lib.nvt_cast_many(None, 1, None), b"null descriptors")
    _refused(lib, lib.nvt_cast_many(desc(I64, I8), 0, None), b"ncols")
    bad = [(I32, I64), (I8, I16), (I16, I32), (I8, I64),            # widening
           (I32, I32), (I64, I64), (F64, F64), (F32, F32),          # same type: the driver's no-op
           (I64, F32), (I64, F64), (I32, F32), (F64, I32), (F32, I8), (F64, I64),   # int <-> float
           (F32, F64), (F32, I16), (U8, I8), (I64, U8), (9, I8), (I64, 9), (-1, I8)]
    for s, d in bad:
        _refused(lib, lib.nvt_cast_many(desc(s, d), 1, None), b"unsupported cast")
    _refused(lib, lib.nvt_cast_many(desc(I64, I8, src=None), 1, None), b"null src/dst")
    _refused(lib, lib.nvt_cast_many(desc(I64, I8, dst=None), 1, None), b"null src/dst")
    _refused(lib, lib.nvt_cast_many(desc(I64, I16, src=p + 4), 1, None), b"aligned")
    _refused(lib, lib.nvt_cast_many(desc(I64, I16, dst=p + 257), 1, None), b"aligned")
    _refused(lib, lib.nvt_cast_many(desc(I32, I8, src=p + 2), 1, None), b"aligned")
    for s, d in [(I32, I8), (I32, I16), (I64, I8), (I64, I16), (I64, I32), (F64, F32)]:
        assert lib.nvt_cast_many(desc(s, d, n=0), 1, None) == 0      # zero rows: no launch


def test_cast_driver_refuses_and_skips_without_a_device():
    from nvtabular_amd import kernels as K

    x = torch.arange(5, dtype=torch.int64)
    assert K.cast_many([(x, torch.int64)])[0] is x                   # same dtype: no launch, no copy
    f = torch.zeros(3, dtype=torch.float32)
    assert K.cast_many([(f, torch.float32)])[0] is f
    assert K.cast_many([]) == []
    for src, dst in [(torch.int64, torch.uint8), (torch.float16, torch.float32), (torch.uint8, torch.int8)]:
        with pytest.raises(TypeError, match="unsupported cast"):
            K.cast_many([(torch.zeros(4, dtype=src), dst)])


# ---- graph.json ---------------------------------------------------------------------------------------
def _roundtrip(op):
    path, to_dict = graph_json._lookup(op)
    params, state = to_dict(op, "/nonexistent")
    params, state = json.loads(json.dumps(params)), json.loads(json.dumps(state))   # what a file holds
    return path, graph_json._entries()[path][2](params, state, "/nonexistent")


def test_graph_json_records_of_the_new_operators():
    op = ops.ReduceDtypeSize(float_dtype=np.float32)
    op.ranges = {"a": (-(2**63), 2**63 - 1), "b": (0, 127), "f": (-1.5, float("inf")), "e": (None, None)}
    op.dtypes = {"a": np.dtype("int64"), "b": np.dtype("int8"), "f": np.dtype("float32"), "e": np.dtype("int32")}
    path, back = _roundtrip(op)
    assert path == "nvtabular.ops.reduce_dtype_size.ReduceDtypeSize" and type(back) is ops.ReduceDtypeSize
    assert back.ranges == op.ranges and back.dtypes == op.dtypes and np.dtype(back.float_dtype) == np.float32
    assert all(isinstance(v, int) for v in back.ranges["a"])          # int64 ends stay exact ints

    st = ops.DataStats()
    st.fit_finalize({"i": {"dtype": "int64", "min": -(2**63), "max": 2**53 + 1, "mean": 0.5, "std": 1.5,
                           "per_nan": 10.0, "cardinality": 7},
                     "f": {"dtype": "float32", "min": -0.5, "max": 2.0, "mean": 0.25, "std": 0.125, "per_nan": 0.0}})
    path, back = _roundtrip(st)
    assert path == "nvtabular.ops.data_stats.DataStats" and back.output == st.output
    assert back.col_names == ["i", "f"] and back.col_types == ["cats", "conts"]

    path, back = _roundtrip(ops.DropLowCardinality(min_cardinality=9))
    assert path == "nvtabular.ops.drop_low_cardinality.DropLowCardinality" and back.min_cardinality == 9

    for op in (ops.AddMetadata(tags=[Tags.TARGET], properties={"a": {"b": 1}}), ops.AddTags([Tags.USER]),
               ops.AddProperties({"k": 2}), ops.TagAsUserID(), ops.TagAsItemID(), ops.TagAsUserFeatures(),
               ops.TagAsItemFeatures()):
        path, back = _roundtrip(op)
        assert path == f"nvtabular.ops.add_metadata.{type(op).__name__}" and type(back) is type(op)
        assert list(back.tags) == list(op.tags) and back.properties == op.properties


def test_saved_workflow_keeps_fitted_state_and_schema(tmp_path):
    red, st = ops.ReduceDtypeSize(), ops.DataStats()
    wf = nvt.Workflow(["u", "x"] >> red >> st >> ops.TagAsUserFeatures())
    wf.fit_schema(_schema())
    red.fit_finalize({"u": (np.dtype("int64"), -5, 300), "x": (np.dtype("float32"), 0.0, 1.0)})
    st.fit_finalize({"u": {"dtype": "int16", "min": -5, "max": 300, "mean": 1.0, "std": 2.0, "per_nan": 0.0,
                           "cardinality": 3}})
    wf.fit_schema(_schema())
    assert wf.output_schema["u"].dtype == np.dtype("int16") and wf.output_schema["x"].dtype == np.dtype("float32")
    wf.save(str(tmp_path))
    back = nvt.Workflow.load(str(tmp_path))
    assert back.output_schema["u"].dtype == np.dtype("int16") and Tags.USER in back.output_schema["x"].tags
    got = {type(n.op).__name__: n.op for n in nvt.node.iter_nodes(back.output_node) if n.op is not None}
    assert got["ReduceDtypeSize"].dtypes == red.dtypes and got["ReduceDtypeSize"].ranges == red.ranges
    assert got["DataStats"].output == st.output


def test_reduce_dtype_size_schema_before_and_after_fit_and_clear():
    red = ops.ReduceDtypeSize()
    wf = nvt.Workflow(["u", "x"] >> red)
    wf.fit_schema(_schema())
    assert [c.dtype for c in wf.output_schema] == [np.dtype("int64"), np.dtype("float32")]   # the input's
    red.fit_finalize({"u": (np.dtype("int64"), 0, 127), "x": (np.dtype("float64"), None, None)})
    assert red.ranges == {"u": (0, 127), "x": (None, None)}
    assert red.dtypes == {"u": np.dtype("int8"), "x": np.dtype("float64")}     # no valid row: unchanged
    red.clear()
    assert red.ranges == {} and red.dtypes == {}


def test_reference_module_aliases():
    import nvtabular  # noqa: F401
    from nvtabular.ops.add_metadata import AddMetadata, TagAsItemID
    from nvtabular.ops.data_stats import DataStats
    from nvtabular.ops.drop_low_cardinality import DropLowCardinality
    from nvtabular.ops.reduce_dtype_size import ReduceDtypeSize

    assert (AddMetadata, TagAsItemID, DataStats, DropLowCardinality, ReduceDtypeSize) == (
        ops.AddMetadata, ops.TagAsItemID, ops.DataStats, ops.DropLowCardinality, ops.ReduceDtypeSize)


# ---- host arithmetic ----------------------------------------------------------------------------------
def test_per_nan_is_the_reference_expression():
    for valid, rows in [(0, 7), (7, 7), (1, 3), (2, 3), (899, 1000), (2**40 + 1, 2**41), (3, 2**53)]:
        s_count, s_len = np.int64(valid), rows
        assert P.per_nan(valid, rows) == float(100 * (1 - s_count / s_len))
    assert math.isnan(P.per_nan(0, 0))
    s = pd.Series([1.0, None, 3.0, None, None, 6.0, 7.0])
    assert P.per_nan(int(s.count()), len(s)) == 100 * (1 - s.count() / len(s))


def test_length_stats_against_pandas():
    words = ["a"] * 5 + ["bcd"] * 2 + ["naïve"] * 3 + ["日本語テキスト"] + [""] * 4
    pairs = [(len(w), c) for w, c in pd.Series(words).value_counts().items()]
    lens = pd.Series(words).str.len()
    lo, hi, mean, std = P.length_stats(pairs)
    assert (lo, hi) == (int(lens.min()), int(lens.max())) and isinstance(lo, int)
    np.testing.assert_allclose([mean, std], [lens.mean(), lens.std()], rtol=1e-14)
    assert P.length_stats([(4, 1)])[:3] == (4, 4, 4.0) and math.isnan(P.length_stats([(4, 1)])[3])
    assert all(math.isnan(v) for v in P.length_stats([]))
    assert all(math.isnan(v) for v in P.length_stats([(3, 0)]))


def test_extrema_keys_merge_like_numpy():
    """The cross-rank fold of fit_end: extrema travel as int64 keys, MIN / MAX of the keys is MIN / MAX
    of the values -- integers exact beyond 2**53, floats with -0.0 < +0.0, +-inf as values, NaN = empty."""
    rng = np.random.default_rng(3)
    ints = np.array([2**63 - 1, -(2**63), 2**53 + 1, -(2**53) - 1, 0, -1, 7], dtype=np.int64)
    flts = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.5, -2.5, 1e308, np.nan])
    is_float = torch.tensor([False] * 6 + [True] * 8)
    ranks = []
    for _ in range(5):
        ext = np.zeros((14, 2), dtype=np.int64)
        ext[:6, 0], ext[:6, 1] = rng.choice(ints, 6), rng.choice(ints, 6)
        ext[5] = (P.INT64_MAX, P.INT64_MIN)                                   # an integer row that saw nothing
        ext[6:, 0] = rng.choice(flts, 8).view(np.int64)
        ext[6:, 1] = rng.choice(flts, 8).view(np.int64)
        ext[13] = np.array([np.nan, np.nan]).view(np.int64)                    # a float row that saw nothing
        ranks.append(ext)
    keys = [P.extrema_to_keys(torch.from_numpy(e), is_float) for e in ranks]
    lo = torch.stack([k[0] for k in keys]).min(dim=0).values
    hi = torch.stack([k[1] for k in keys]).max(dim=0).values
    got = P.keys_to_extrema(lo, hi, is_float).numpy()
    all_ext = np.stack(ranks)
    np.testing.assert_array_equal(got[:6, 0], all_ext[:, :6, 0].min(axis=0))
    np.testing.assert_array_equal(got[:6, 1], all_ext[:, :6, 1].max(axis=0))
    assert got[5].tolist() == [P.INT64_MAX, P.INT64_MIN]
    f = all_ext[:, 6:, :].copy().view(np.float64)
    for j in range(8):
        for side, pick in ((0, min), (1, max)):
            vals = [v for v in f[:, j, side].tolist() if v == v]
            g = got[6 + j, side:side + 1].view(np.float64)[0]
            if not vals:
                assert math.isnan(g)
                continue
            # total order: by value, -0.0 below +0.0
            best = pick(vals, key=lambda v: (v, not math.copysign(1, v) < 0))
            assert g == best and math.copysign(1, g) == math.copysign(1, best), (j, side, vals, g)
    # the transformation is its own inverse on every row
    for e in ranks:
        back = P.keys_to_extrema(*P.extrema_to_keys(torch.from_numpy(e), is_float), is_float).numpy()
        np.testing.assert_array_equal(back, e)


def test_profile_rows_decodes_exact_ints_and_floats():
    from nvtabular_amd import kernels as K

    host = np.zeros((3, K.PROFILE_WORDS), dtype=np.int64)
    host[0] = [10, 4, -(2**53) - 1, 2**63 - 1, *np.array([1.5, 2.25]).view(np.int64)]
    host[1] = [10, 2, *np.array([-0.0, np.inf, 3.0, 9.0]).view(np.int64)]
    host[2] = [5, 0, 2**63 - 1, -(2**63), 0, 0]
    rows = K.profile_rows(host, [torch.int64, torch.float32, torch.int32])
    assert rows[0] == dict(rows=10, valid=4, min=-(2**53) - 1, max=2**63 - 1, sum=1.5, sumsq=2.25)
    assert isinstance(rows[0]["min"], int)
    assert rows[1]["max"] == np.inf and math.copysign(1, rows[1]["min"]) == -1 and rows[1]["sum"] == 3.0
    assert rows[2]["min"] is None and rows[2]["max"] is None and rows[2]["valid"] == 0
