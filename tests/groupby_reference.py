"""Plain numpy references of what csrc/nvt_groupby.hip computes for ``K.GroupbyTable`` (the hash-table
groupby of 1..3 int64 key columns: update, merge, compact, index_build, lookup), csrc/nvt_order_rows.hip
for ``K.order_rows`` (sort-key images + stable radix refinement) and csrc/nvt_segreduce.hip for
``K.seg_aggregate`` (segmented reduction over rows ordered by group), for the kernel-level tests of
test_gpu_groupby_kernels.py.
test_groupby_reference.py pins them to pandas on the CPU.  Nothing here shares code with the
device side: grouping is ``np.lexsort`` + ``ufunc.reduceat`` in float64, orders are value ranks
from ``np.unique`` fed to a stable ``np.argsort`` (never a bit image of the value).

Validity is a bool array or None (all valid) everywhere; the device tests pack it into bitmaps.
Values are reduced as float64, the contract of include/nvt_hip.h for every value dtype.
"""
import numpy as np

from encode_reference import first_mismatch, pack_bits  # noqa: F401  (re-exported for the tests)

I64_MIN, I64_MAX = -(2**63), 2**63 - 1


def _ok(valid, n):
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, dtype=bool)
    assert ok.shape == (n,)
    return ok


def entries(v, valid):
    """(values as float64, mask of the entries that count: valid and not NaN)."""
    v = np.asarray(v)
    x = v.astype(np.float64)
    return x, _ok(valid, v.size) & ~np.isnan(x)


def _runs(cols):
    """Rows ordered by the tuple ``cols`` (most significant first): (order, start of every run of
    equal tuples in that order)."""
    n = cols[0].size
    order = np.lexsort(tuple(reversed(cols)))
    if n == 0:
        return order, np.zeros(0, np.int64)
    head = np.zeros(n, bool)
    head[0] = True
    for c in cols:
        s = c[order]
        head[1:] |= s[1:] != s[:-1]
    return order, np.flatnonzero(head)


def _stats(order, starts, cols, sumsq, minmax):
    """Per run: sum / sumsq / min / max of every (float64 values, counting mask) column."""
    g = starts.size
    out = dict(sum=[], sumsq=[] if sumsq else None, min=[] if minmax else None,
               max=[] if minmax else None, nvalid=[])
    for x, ok in cols:
        xs, oks = x[order], ok[order]
        red = lambda uf, a: uf.reduceat(a, starts) if g else np.zeros(0, a.dtype)  # noqa: E731
        z = np.where(oks, xs, 0.0)
        out["sum"].append(red(np.add, z))
        out["nvalid"].append(red(np.add, oks.astype(np.int64)))
        if sumsq:
            out["sumsq"].append(red(np.add, z * z))
        if minmax:
            none = out["nvalid"][-1] == 0
            lo = red(np.minimum, np.where(oks, xs, np.inf))
            hi = red(np.maximum, np.where(oks, xs, -np.inf))
            out["min"].append(np.where(none, np.nan, lo))
            out["max"].append(np.where(none, np.nan, hi))
    return out


def table_groups(keys, key_valid, vals, val_valid, sumsq=False, minmax=False):
    """The groups of ``K.GroupbyTable.update`` + ``compact`` over these rows, ordered by
    (null_mask, key tuple).

    * a null key component is a value of its own (pandas ``dropna=False``): bit k of ``null_mask``
      is set and ``keys[k]`` holds 0, whatever bytes lie under the null;
    * ``size`` counts rows, ``count`` rows whose FIRST key component is non-null;
    * sum / sumsq / min / max run over the entries of a value column that are valid and not NaN;
      min / max are NaN for a group without such an entry (a group of infinities keeps them);
    * ``row_group``: every row's index into the group arrays.
    """
    nk = len(keys)
    n = np.asarray(keys[0]).size
    key_valid = key_valid if key_valid is not None else [None] * nk
    val_valid = val_valid if val_valid is not None else [None] * len(vals)
    nm = np.zeros(n, np.int64)
    stored = []
    for k in range(nk):
        ok = _ok(key_valid[k], n)
        nm |= (~ok).astype(np.int64) << k
        stored.append(np.where(ok, np.asarray(keys[k]).astype(np.int64), 0))
    order, starts = _runs([nm] + stored)
    first = order[starts]
    size = np.diff(np.append(starts, n)).astype(np.int64)
    mask = nm[first]
    out = _stats(order, starts, [entries(v, w) for v, w in zip(vals, val_valid)], sumsq, minmax)
    row_group = np.empty(n, np.int64)
    row_group[order] = np.repeat(np.arange(starts.size), size)
    out.update(keys=[s[first] for s in stored], null_mask=mask.astype(np.uint8), size=size,
               count=np.where(mask & 1, 0, size), n=int(starts.size), row_group=row_group)
    return out


def merge_groups(a, b):
    """Two ``table_groups`` results (or compacted tables) as one: sizes, counts, sums and sums of
    squares add, min / max combine skipping NaN (NaN only where both sides are NaN)."""
    nk = len(a["keys"])
    cat = lambda f: np.concatenate([np.asarray(f(a)), np.asarray(f(b))])  # noqa: E731
    keys = [cat(lambda d, k=k: d["keys"][k]).astype(np.int64) for k in range(nk)]
    nm = cat(lambda d: d["null_mask"]).astype(np.int64)
    order, starts = _runs([nm] + keys)
    red = lambda uf, x: uf.reduceat(x[order], starts) if starts.size else x[:0]  # noqa: E731
    nv = len(a["sum"])
    has = lambda f: a.get(f) is not None and b.get(f) is not None  # noqa: E731
    col = lambda f, uf: [red(uf, cat(lambda d, j=j: d[f][j])) for j in range(nv)]  # noqa: E731
    first = order[starts]
    return dict(keys=[k[first] for k in keys], null_mask=nm[first].astype(np.uint8),
                size=red(np.add, cat(lambda d: d["size"]).astype(np.int64)),
                count=red(np.add, cat(lambda d: d["count"]).astype(np.int64)),
                sum=col("sum", np.add), sumsq=col("sumsq", np.add) if has("sumsq") else None,
                min=col("min", np.fmin) if has("min") else None,
                max=col("max", np.fmax) if has("max") else None, n=int(starts.size))


def lookup(group_keys, group_null_mask, keys, key_valid):
    """Index of every row's key tuple in the group arrays, -1 where the tuple is no group.  A null
    component matches only a group whose null mask has that bit."""
    nk = len(keys)
    n = np.asarray(keys[0]).size
    key_valid = key_valid if key_valid is not None else [None] * nk
    table = {}
    gm = np.asarray(group_null_mask).astype(np.int64).tolist()
    for g, tup in enumerate(zip(gm, *[np.asarray(k).tolist() for k in group_keys])):
        assert table.setdefault(tup, g) == g, f"group {g} repeats the tuple of group {table[tup]}"
    nm = np.zeros(n, np.int64)
    stored = []
    for k in range(nk):
        ok = _ok(key_valid[k], n)
        nm |= (~ok).astype(np.int64) << k
        stored.append(np.where(ok, np.asarray(keys[k]).astype(np.int64), 0).tolist())
    return np.array([table.get(t, -1) for t in zip(nm.tolist(), *stored)], np.int64).reshape(n)


def _ranks(values, valid, ascending):
    """Dense rank of every row in the column's order; nulls and NaN share the last rank.

    The contract of nvt_sort_key_u64 (include/nvt_hip.h): the key is 64 bits wide and its largest
    image is reserved for nulls, so the two int64 values at the far end of the order -- INT64_MAX
    and INT64_MAX - 1 ascending, INT64_MIN and INT64_MIN + 1 descending -- rank EQUAL.  Narrower
    integers and floats never get there.  -0.0 and +0.0 are equal (``np.unique`` compares)."""
    v = np.asarray(values)
    if v.dtype == np.bool_:
        v = v.view(np.uint8)
    n = v.size
    ok = _ok(valid, n)
    if v.dtype.kind == "f":
        ok = ok & ~np.isnan(v)
        v = v.astype(np.float64)
    else:
        v = v.astype(np.int64)
        v = np.minimum(v, I64_MAX - 1) if ascending else np.maximum(v, I64_MIN + 1)
    uniq, inv = np.unique(v[ok], return_inverse=True)
    rank = np.full(n, uniq.size, np.int64)
    rank[ok] = inv if ascending else uniq.size - 1 - inv
    return rank


def sort_key_order(cols, ascending=True):
    """Stable lexicographic row order of ``cols`` = [(values, valid), ...], most significant first;
    ``ascending`` is one bool or one per column.  Nulls and NaN last in either direction, ties
    (-0.0 against +0.0 among them) in row order."""
    n = np.asarray(cols[0][0]).size
    asc = [ascending] * len(cols) if isinstance(ascending, (bool, np.bool_)) else list(ascending)
    assert len(asc) == len(cols)
    order = np.arange(n, dtype=np.int64)
    for (values, valid), up in reversed(list(zip(cols, asc))):   # least significant first
        rank = _ranks(values, valid, bool(up))
        order = order[np.argsort(rank[order], kind="stable")]
    return order


def order_rows(n, sort_cols=(), ascending=True, gid=None, ngroups=0):
    """``K.order_rows``: rows ordered by the sort columns, then stably by group id (-1 = null key,
    behind every group).  int64 words, row index in the low 32 bits; with ``gid`` the high half is
    the group id, ``ngroups`` for the rows of null keys (without it the high half is 0 here and
    unspecified on the device)."""
    order = sort_key_order(list(sort_cols), ascending) if len(sort_cols) else np.arange(n, dtype=np.int64)
    assert order.size == n
    if gid is None:
        return order
    g = np.asarray(gid).astype(np.int64)
    assert g.shape == (n,) and (n == 0 or (g.min() >= -1 and g.max() < ngroups))
    g = np.where(g < 0, ngroups, g)
    order = order[np.argsort(g[order], kind="stable")]
    return (g[order] << 32) | order


def seg_aggregate(words, ngroups, vals, val_valid, sumsq=False, minmax=False):
    """``K.seg_aggregate``: (size [G], count [V, G], sum, sumsq or None, min or None, max or None)
    of the words (group << 32 | row).  Words whose group is >= ngroups are ignored; a group
    without a counting entry keeps the initial values 0 / 0 / 0 / 0 / +inf / -inf.  The words need
    not be ordered here (the device wants them ordered by group)."""
    words = np.asarray(words).astype(np.int64)
    grp, row = words >> 32, words & 0xFFFFFFFF
    keep = grp < ngroups
    grp, row = grp[keep], row[keep]
    val_valid = val_valid if val_valid is not None else [None] * len(vals)
    nv = len(vals)
    size = np.bincount(grp, minlength=ngroups).astype(np.int64)
    order, starts = _runs([grp])
    ids = grp[order[starts]]
    cols = []
    for v, w in zip(vals, val_valid):
        x, ok = entries(v, w)
        cols.append((x[row], ok[row]))
    st = _stats(order, starts, cols, sumsq, minmax)

    def spread(parts, init, dtype=np.float64):
        out = np.full((nv, ngroups), init, dtype)
        for j, p in enumerate(parts):
            some = st["nvalid"][j] > 0
            out[j, ids[some]] = p[some]
        return out

    sumsq, minmax = bool(sumsq and nv), bool(minmax and nv)     # (no columns: no lists, as K.seg_aggregate)
    return (size, spread(st["nvalid"], 0, np.int64), spread(st["sum"], 0.0),
            spread(st["sumsq"], 0.0) if sumsq else None,
            spread(st["min"], np.inf) if minmax else None,
            spread(st["max"], -np.inf) if minmax else None)


def split_by_group(values, valid, group, ngroups):
    """The counting entries (float64) of a value column per group, in row order: a list of
    ``ngroups`` arrays (rows with group < 0 belong to none)."""
    x, ok = entries(values, valid)
    group = np.asarray(group)
    idx = np.flatnonzero(ok & (group >= 0))
    idx = idx[np.argsort(group[idx], kind="stable")]
    cuts = np.searchsorted(group[idx], np.arange(1, ngroups))
    return np.split(x[idx], cuts)


def sort_groups(comp):
    """A compacted table (dict of host arrays, any order) in the order of ``table_groups``."""
    order = np.lexsort(tuple(reversed([np.asarray(comp["null_mask"]).astype(np.int64)]
                                      + [np.asarray(k) for k in comp["keys"]])))
    take = lambda x: None if x is None else [np.asarray(c)[order] for c in x]  # noqa: E731
    return dict(keys=take(comp["keys"]), null_mask=np.asarray(comp["null_mask"])[order],
                size=np.asarray(comp["size"])[order], count=np.asarray(comp["count"])[order],
                sum=take(comp["sum"]), sumsq=take(comp.get("sumsq")), min=take(comp.get("min")),
                max=take(comp.get("max")), n=int(order.size))


def assert_same_groups(got, exp, what, sumsq=True, minmax=True):
    """Two group dicts in the order of ``table_groups``, field by field, exactly (NaN equals NaN).
    An absent list is None or empty; ``sumsq`` / ``minmax`` False: the field must be absent in
    ``got`` and is not looked at in ``exp``."""
    assert got["n"] == exp["n"], f"{what}: {got['n']} groups, expected {exp['n']}"
    for k, (a, b) in enumerate(zip(got["keys"], exp["keys"])):
        first_mismatch(np.asarray(a), np.asarray(b), f"{what}: key {k}")
    first_mismatch(np.asarray(got["null_mask"]), np.asarray(exp["null_mask"]), f"{what}: null mask")
    first_mismatch(np.asarray(got["size"]), np.asarray(exp["size"]), f"{what}: size")
    first_mismatch(np.asarray(got["count"]), np.asarray(exp["count"]), f"{what}: count")
    nv = len(got["sum"])
    for f, on in (("sum", True), ("sumsq", sumsq), ("min", minmax), ("max", minmax)):
        if not on:
            assert not got.get(f), f"{what}: {f} present"
            continue
        assert len(got[f]) == nv and len(exp[f]) >= nv, f"{what}: {f} has {len(got[f])} columns"
        for j in range(nv):
            np.testing.assert_array_equal(got[f][j], exp[f][j], err_msg=f"{what}: {f}[{j}]")
