"""Kernel-level matrix for nvt_compact_keep_terms (keep_terms_kernel on produce_tiles,
nvtabular_amd/csrc/nvt_compact.hip), the keep-mask producer of ``Dataset(filters=...)``.  The entry
point is called through ``_lib.load()`` on buffers this file owns; the plan lies between 256-byte
guards of 0xA5, which must be intact afterwards.  The mask words (with the bits past n) and the tile
counts are compared bit for bit with filter_terms_reference.py (pinned to pyarrow on the CPU by
test_filter_terms_reference.py), then nvt_compact_plan must give the exclusive scan and m.

Branch or property -> the case that reaches it (a tile is 2048 rows = 32 mask words; a wave is 64 rows).

  the last word short, a second / fourth tile     n = 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17   test_dtypes_and_operators
  every column dtype, with and without a bitmap   float32 .. int16, one term of every operator          test_dtypes_and_operators
  a null fails all but `not in`                   bitmaps with about a fifth of the rows null             test_dtypes_and_operators
  1 term / 64 terms, 1 column / 16 columns        shapes "1x64", "64x1", "mixed" over 1 and 16 columns   test_shapes, test_dtypes_and_operators
  set runs of 0, 1, 2 and 4097 words              `in` and `not in`, int64 and float64 columns           test_set_lengths
  the wave-level skip of a dead conjunction       a first term false for a whole wave, true for a whole  test_wave_placement
                                                  wave, mixed inside a wave; a later conjunction revives
  the reuse of the value just loaded              two adjacent terms on one column, then another column, test_adjacent_terms
                                                  then the first again (reloaded), across conjunctions
  NaN, -0.0, 0.0 in both float widths             as values and as constants, in sets too                 test_special_values
  INT64_MIN / INT64_MAX                           as values and as constants, in sets too                 test_special_values
  the descriptors filters.py lowers a DNF to      term order, sorted distinct sets, string surrogates    test_lowered_descriptors
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import compact_reference as CR
import filter_terms_reference as R
from kernel_buffers import Guarded, Lib, dev

pytestmark = pytest.mark.gpu

CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3,
        np.dtype(np.uint8): 4, np.dtype(np.int8): 5, np.dtype(np.int16): 6}       # NVT_F32 .. NVT_I16
DTYPES = list(CODE)
OPC = {op: i for i, op in enumerate(R.OPS)}                                         # NVT_FILTER_EQ ..
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def L():
    lib = Lib()
    assert [lib.m.NVT_F32, lib.m.NVT_F64, lib.m.NVT_I32, lib.m.NVT_I64, lib.m.NVT_U8, lib.m.NVT_I8,
            lib.m.NVT_I16] == list(CODE.values())
    assert lib.m.FILTER_OPS == OPC and (lib.m.FILTER_MAX_COLS, lib.m.FILTER_MAX_TERMS) == (16, 64)
    yield lib
    torch.cuda.empty_cache()


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def run(L, cols, terms, n, what=""):
    """cols: [(values, valid bool[] or None)]; terms: [(col, op, conj, constant)] sorted by conj, a
    list as the constant of `in` / `not in`.  Builds the descriptors by hand, calls the producer and
    nvt_compact_plan, and compares with the reference; returns the keep mask."""
    keep_alive, descs = [], (L.m.FilterCol * len(cols))()
    for d, (x, valid) in zip(descs, cols):
        t = dev(x)
        v = None if valid is None else dev(CR.pack_bits(valid))
        keep_alive.append((t, v))
        d.x, d.valid, d.dtype = t.data_ptr(), None if v is None else v.data_ptr(), CODE[x.dtype]
    tdesc = (L.m.FilterTerm * len(terms))()
    runs, off = [], 0
    for d, (j, op, conj, const) in zip(tdesc, terms):
        flt = cols[j][0].dtype.kind == "f"
        d.col, d.op, d.conj = j, OPC[op], conj
        if op in ("in", "not in"):
            vals = np.unique(np.asarray(const, dtype=np.float64) + 0.0) if flt else \
                np.unique(np.asarray(const, dtype=np.int64))
            vals = vals[~np.isnan(vals)] if flt else vals
            d.set_off, d.set_len = off, len(vals)
            runs.append(vals.view(np.uint64))
            off += len(vals)
        elif flt:
            d.value.f = float(const)
        else:
            d.value.i = int(const)
    words = np.concatenate(runs) if runs else np.zeros(0, dtype=np.uint64)
    sets = Guarded(words.nbytes, init=words) if words.size else None

    dnf = {}
    for j, op, conj, const in terms:
        dnf.setdefault(conj, []).append((j, op, const))
    keep = R.keep_mask(list(dnf.values()), dict(enumerate(cols)), n)

    need = C.c_uint64()
    L.m.check(L.lib.nvt_compact_ws_bytes(n, C.byref(need)), "nvt_compact_ws_bytes")
    at_words, at_base, end_base = CR.plan_layout(n)
    plan = Guarded(need.value, guard=256)
    L.call("nvt_compact_keep_terms", descs, len(cols), tdesc, len(terms), None if sets is None else sets.ptr,
           int(words.size), n, plan.ptr, need.value)
    raw = plan.read(what=what + ": plan")
    want_words, want_counts = R.plan(keep)
    np.testing.assert_array_equal(raw[at_words: at_base].view(np.uint64), want_words, err_msg=what + ": mask words")
    base = raw[at_base: end_base].view(np.uint32)
    np.testing.assert_array_equal(base[:-1], want_counts, err_msg=what + ": tile counts")
    assert base[-1] == 0, what
    if sets is not None:
        np.testing.assert_array_equal(sets.read(np.uint64, what + ": sets"), words)

    out_m = Guarded(8)
    L.call("nvt_compact_plan", n, plan.ptr, need.value, out_m.ptr)
    raw = plan.read(what=what + ": plan after the scan")
    np.testing.assert_array_equal(raw[at_words: at_base].view(np.uint64), want_words, err_msg=what + ": words after scan")
    np.testing.assert_array_equal(raw[at_base: end_base].view(np.uint32), CR.plan(keep)[2], err_msg=what + ": bases")
    assert int(out_m.read(np.uint64, "out_m")[0]) == int(keep.sum()), what
    return keep


def column(rng, dt, n, bitmap, lo=-6, hi=7):
    dt = np.dtype(dt)
    if dt.kind == "f":
        x = (rng.integers(lo, hi, n) * 0.5).astype(dt)
        x[rng.random(n) < 0.05] = np.nan
    elif dt == np.uint8:
        x = rng.integers(0, hi, n).astype(dt)
    else:
        x = rng.integers(lo, hi, n).astype(dt)
    return x, (rng.random(n) >= 0.2 if bitmap else None)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bitmap", [False, True], ids=["dense", "bitmap"])
@pytest.mark.parametrize("n", SIZES)
def test_dtypes_and_operators(L, n, bitmap):
    rng = np.random.default_rng(seed_of("ops", n, bitmap))
    kept = 0
    for dt in DTYPES:
        col = column(rng, dt, n, bitmap)
        for op in R.OPS:
            const = [1, -2, 3, 1] if op in ("in", "not in") else 1
            if np.dtype(dt) == np.uint8 and op in ("in", "not in"):
                const = [1, 2, 3, 1]
            kept += run(L, [col], [(0, op, 0, const)], n, f"{np.dtype(dt)} {op} n={n}").sum()
    assert kept > 0


LO, HI = -40, 41          # the values of test_shapes: integers, or halves of them in the float columns


def shape_terms(rng, shape, ncols):
    """64 terms: one conjunction of 64 weak terms, 64 conjunctions of one selective term, or a mix."""
    sizes = {"1x64": [64], "64x1": [1] * 64, "mixed": [1, 5, 20, 2, 36]}[shape]
    terms = []
    for conj, size in enumerate(sizes):
        weak = size > 2
        for k in range(size):
            j = int(rng.integers(0, ncols))
            if weak:
                op = ["!=", ">=", "<=", "not in", "in", ">", "<"][k % 7]
                const = {"!=": int(rng.integers(LO, HI)), ">=": LO, "<=": HI - 1, ">": LO - 1, "<": HI,
                         "not in": [int(rng.integers(LO, HI))], "in": list(range(LO, HI - 2))}[op]
            else:
                op = ["==", "in", "<", ">"][int(rng.integers(0, 4))]
                const = {"==": int(rng.integers(LO, HI)), "in": [int(v) for v in rng.integers(LO, HI, 2)],
                         "<": LO + 2, ">": HI - 3}[op]
            terms.append((j, op, conj, const))
    return terms


@pytest.mark.parametrize("n", [65, 3 * 2048 + 17])
@pytest.mark.parametrize("ncols", [1, 16])
@pytest.mark.parametrize("shape", ["1x64", "64x1", "mixed"])
def test_shapes(L, shape, ncols, n):
    rng = np.random.default_rng(seed_of("shape", shape, ncols, n))
    dts = [np.int64, np.float32, np.int16, np.float64, np.int8, np.int32]
    cols = [column(rng, dts[j % len(dts)], n, j % 3 == 1, LO, HI) for j in range(ncols)]
    terms = shape_terms(rng, shape, ncols)
    assert len(terms) == 64
    keep = run(L, cols, terms, n, f"{shape} over {ncols} columns, n={n}")
    if n > 1000:
        assert 0 < keep.sum() < n


@pytest.mark.parametrize("dt", [np.int64, np.float64, np.float32], ids=["int64", "float64", "float32"])
@pytest.mark.parametrize("length", [0, 1, 2, 4097])
def test_set_lengths(L, length, dt):
    n = 2049
    rng = np.random.default_rng(seed_of("sets", length, np.dtype(dt)))
    x = rng.integers(0, 10000, n).astype(dt)
    if np.dtype(dt).kind == "f":
        x[:3] = [np.nan, -0.0, 0.0]
    valid = rng.random(n) >= 0.1
    members = [int(v) for v in rng.permutation(10000)[:length]]      # (distinct: the run has `length` words)
    other = column(rng, np.int32, n, False)
    for op in ("in", "not in"):
        keep = run(L, [(x, valid), other], [(0, op, 0, members)], n, f"{op} a set of {length}")
        if length == 0:
            assert keep.sum() == (0 if op == "in" else n)    # (a null passes `not in`)
        if length == 4097:
            assert 0 < keep.sum() < n
        # the run of the second term starts behind the first one's
        run(L, [(x, valid), other], [(1, "in", 0, [1, 2]), (0, op, 0, members), (1, "not in", 1, [0])], n,
            f"{op} a set of {length} between two runs")


def test_wave_placement(L):
    """Conjunction 0 = (a == 1) and (b < 4) and (b > -4): a is 0 for the whole of waves 0 and 4 (the
    conjunction dies there and its other terms are skipped), 1 for the whole of waves 1 and 5, mixed
    in the others; conjunction 1 = (c in ...) must still be evaluated everywhere, b reloaded."""
    n = 2048 + 6 * 64 + 9
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2, n).astype(np.int8)
    for t0 in (0, 2048):
        a[t0: t0 + 64] = 0
        a[t0 + 64: t0 + 128] = 1
    b = column(rng, np.float32, n, True)
    c = column(rng, np.int64, n, False)
    terms = [(0, "==", 0, 1), (1, "<", 0, 2.0), (1, ">", 0, -2.0), (2, "in", 1, [5, -5]), (1, "!=", 1, 0.5)]
    keep = run(L, [(a, None), b, c], terms, n, "wave placement")
    assert keep[:64].sum() < keep[64:128].sum()
    # every conjunction dead for whole waves: their words are 0
    a2 = a.copy()
    a2[128:] = 0
    keep = run(L, [(a2, None), b], [(0, "==", 0, 1), (1, "<", 0, 2.0), (0, "==", 1, 1), (1, ">", 1, 0.0)], n,
               "all conjunctions dead")
    assert not keep[:64].any() and not keep[128:].any() and keep[64:128].any()


def test_adjacent_terms(L):
    n = 2049
    rng = np.random.default_rng(12)
    cols = [column(rng, np.int32, n, True), column(rng, np.float64, n, True), column(rng, np.int16, n, False)]
    terms = [(0, ">=", 0, -2), (0, "<=", 0, 3), (1, "<", 0, 1.5), (0, "!=", 0, 0),          # 0, 0, 1, 0 again
             (1, ">", 1, 0.0), (1, "not in", 1, [1.0, 2.5]), (2, "==", 1, 2),
             (2, "in", 2, [1, 2, 3]), (2, "!=", 2, 2), (0, "<", 2, 0)]
    keep = run(L, cols, terms, n, "adjacent terms")
    assert 0 < keep.sum() < n


def test_special_values(L):
    n = 130
    specials_f = [np.nan, -0.0, 0.0, 1.0, -1.0, np.inf, -np.inf, 0.1]
    for dt in (np.float32, np.float64):
        x = np.resize(np.asarray(specials_f, dtype=dt), n)
        valid = np.ones(n, dtype=bool)
        valid[::7] = False
        for const in (np.nan, -0.0, 0.0, 0.1, float(np.float32(0.1)), np.inf):
            for op in R.OPS[:6]:
                run(L, [(x, valid)], [(0, op, 0, const)], n, f"{np.dtype(dt)} {op} {const}")
        for members in ([-0.0], [0.0, 1.0], [np.nan, -1.0], [0.1], [float(np.float32(0.1)), np.inf]):
            for op in ("in", "not in"):
                run(L, [(x, valid)], [(0, op, 0, members)], n, f"{np.dtype(dt)} {op} {members}")
    x = np.resize(np.asarray([I64_MIN, I64_MAX, 0, -1, 1, I64_MIN + 1, I64_MAX - 1], dtype=np.int64), n)
    valid = np.ones(n, dtype=bool)
    valid[::5] = False
    for const in (I64_MIN, I64_MAX, 0, I64_MIN + 1, I64_MAX - 1):
        for op in R.OPS[:6]:
            keep = run(L, [(x, valid)], [(0, op, 0, const)], n, f"int64 {op} {const}")
        assert keep.any()
    for members in ([I64_MIN], [I64_MAX, I64_MIN], [I64_MAX - 1, 0, I64_MIN + 1]):
        for op in ("in", "not in"):
            run(L, [(x, valid)], [(0, op, 0, members)], n, f"int64 {op} {members}")


def test_lowered_descriptors(L):
    """The descriptors filters.py lowers a DNF to, run through the kernel: the terms of a column made
    adjacent inside a conjunction, sets sorted and distinct, a string constant as its surrogate, a
    datetime constant as its count, a bool as 0 / 1."""
    import pandas as pd

    from nvtabular_amd import filters as F
    from nvtabular_amd.schema import Schema
    from nvtabular_amd.strings import string_key64

    n = 2 * 2048 + 5
    rng = np.random.default_rng(13)
    words = np.array(["a", "b", "", "zebra"], dtype=object)
    df = pd.DataFrame({
        "i": rng.integers(-5, 6, n).astype(np.int32),
        "f": (rng.integers(-8, 9, n) * 0.25).astype(np.float32),
        "s": words[rng.integers(0, 4, n)],
        "t": (np.datetime64("2024-01-01", "ms") + rng.integers(0, 6, n) * np.timedelta64(12, "h")),
        "b": rng.random(n) < 0.5,
    })
    dnf = [[("i", ">", -3), ("s", "in", ["zebra", "a", "a"]), ("i", "<=", 4.0), ("f", "not in", [0.5, -0.0, 0.5])],
           [("t", ">=", pd.Timestamp("2024-01-02")), ("b", "==", True), ("s", "!=", "b"), ("t", "<", np.datetime64("2024-01-03"))],
           [("f", "in", [])]]
    flt = F.validate(F.normalize(dnf), Schema.from_frame(df))
    assert [[t.column for t in conj] for conj in flt.dnf] == [["i", "i", "s", "f"], ["s", "t", "t", "b"], ["f"]]
    unit = np.datetime_data(df["t"].dtype)[0]                        # (what the column holds on the device)
    stamps = df["t"].to_numpy().astype(f"datetime64[{unit}]")
    device = {"i": df["i"].to_numpy(), "f": df["f"].to_numpy(), "s": string_key64(df["s"].to_numpy()),
              "t": stamps.view(np.int64), "b": df["b"].to_numpy().view(np.uint8)}
    low = flt.lower({c: device[c].dtype.kind == "f" for c in flt.columns})
    assert low.columns == ["i", "s", "f", "t", "b"]
    for (j, op, conj, set_len, set_off, value) in low.terms:
        run_words = low.sets[set_off: set_off + set_len]
        vals = run_words.view(np.float64 if low.floats[j] else np.int64)
        assert (np.diff(vals) > 0).all()
    cols = [(device[c], None) for c in low.columns]
    terms = []
    for (j, op, conj, set_len, set_off, value) in low.terms:
        if R.OPS[op] in ("in", "not in"):
            value = list(low.sets[set_off: set_off + set_len].view(np.float64 if low.floats[j] else np.int64))
        terms.append((j, R.OPS[op], conj, value))
    keep = run(L, cols, terms, n, "lowered")
    # ... and those are the rows the DNF keeps on the frame itself
    frame = {c: (df[c].to_numpy(), None) for c in df.columns}
    frame["t"] = (stamps, None)
    np.testing.assert_array_equal(keep, R.keep_mask(dnf, frame, n))
    assert 0 < keep.sum() < n
