"""Plain numpy references of the hash join against an external table, for the kernel-level tests of
csrc/nvt_join.hip and the scan of csrc/nvt_scan.hpp (test_gpu_join_kernels.py).
test_join_reference.py pins the composed reference

    canon -> group_rows -> probe -> exclusive_offsets -> expand -> gather

to ``pandas.merge`` on the CPU.  Nothing here shares code with the device side: keys are looked up
in a Python dict, rows are expanded with ``np.repeat``, offsets are a ``np.cumsum`` in uint64.  The
contract followed is the one of include/nvt_hip.h, "hash join against an external table"; the hash
is the public one of DESIGN.md section 4 (murmur3 fmix64, home slot = hash & (capacity - 1)).  The
fingerprint of a key of 2 to 4 components is internal to the kernels and is not restated here.
"""
import numpy as np

JOIN_INT, JOIN_FLOAT = 0, 1
U64 = np.uint64
MASK64 = (1 << 64) - 1


def pack_bits(bits) -> np.ndarray:
    """Arrow validity bitmap (LSB first) of a boolean array: bit i set = row i valid."""
    return np.packbits(np.asarray(bits, dtype=bool), bitorder="little")


def pack_words(bits) -> np.ndarray:
    """The same bitmap in whole 64-bit words: ceil(n / 64) * 8 bytes, bits past n are 0."""
    bits = np.asarray(bits, dtype=bool)
    out = np.zeros((bits.size + 63) // 64 * 8, np.uint8)
    p = pack_bits(bits)
    out[:p.size] = p
    return out


def unpack_bits(bitmap, n) -> np.ndarray:
    return np.unpackbits(np.asarray(bitmap, dtype=np.uint8), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------
def canon(values, dtype, mode, valid_bool):
    """(words uint64, null bool) of one key component.

    JOIN_INT: the sign-extended value (uint8 is zero-extended).  JOIN_FLOAT: the bit pattern of the
    float64 value, -0.0 folded to +0.0; integers are converted with ``astype(float64)``, float32 is
    widened.  Null: a cleared validity bit or any NaN; the word is then 0."""
    dtype = np.dtype(dtype)
    x = np.asarray(values).astype(dtype, copy=False)
    n = x.size
    null = np.zeros(n, bool) if valid_bool is None else ~np.asarray(valid_bool, dtype=bool)
    if mode == JOIN_FLOAT:
        with np.errstate(invalid="ignore"):           # (widening a signalling float32 NaN)
            d = x.astype(np.float64)
        null = null | np.isnan(d)
        d = np.where(d == 0.0, 0.0, d)
        words = d.view(U64).copy()
    else:
        assert mode == JOIN_INT and dtype.kind in "iu", "a float key column needs JOIN_FLOAT"
        words = x.astype(np.int64).view(U64).copy()
    words[null] = 0
    return words, null


def canon_many(cols, valid_bools, modes):
    """(words uint64 [nkeys][n], nulls uint8 [n]; bit k = component k) of a key of several columns."""
    ws, nulls = [], None
    for k, (x, v, mode) in enumerate(zip(cols, valid_bools, modes)):
        w, nl = canon(x, np.asarray(x).dtype, mode, v)
        ws.append(w)
        bit = nl.astype(np.uint8) << np.uint8(k)
        nulls = bit if nulls is None else nulls | bit
    return np.stack(ws), nulls


def fmix64(x) -> np.ndarray:
    """murmur3's 64-bit finaliser on a uint64 array."""
    h = np.array(x, dtype=U64, ndmin=1, copy=True)
    h ^= h >> U64(33)
    h *= U64(0xFF51AFD7ED558CCD)
    h ^= h >> U64(33)
    h *= U64(0xC4CEB9FE1A85EC53)
    h ^= h >> U64(33)
    return h


def home_slot(tag, capacity) -> np.ndarray:
    assert capacity >= 2 and capacity & (capacity - 1) == 0
    return fmix64(tag) & U64(capacity - 1)


# ---------------------------------------------------------------------------------------------
# the external side
# ---------------------------------------------------------------------------------------------
def group_rows(tags, nulls, nkeys):
    """The stable grouping of kernels_join.ExternalIndex: rows ordered by tag (as int64), external
    order within a key; one component: the null rows last, as one group outside the table.

    -> (order, group_tags uint64, first uint32, count uint32, (null_first, null_count))."""
    tags = np.asarray(tags, dtype=U64)
    nulls = np.asarray(nulls, dtype=np.uint8)
    n = tags.size
    order = np.argsort(tags.view(np.int64), kind="stable")
    if nkeys == 1:
        order = order[np.argsort(nulls[order] != 0, kind="stable")]
    st, sn = tags[order], nulls[order]
    new = np.ones(n, bool)
    new[1:] = (st[1:] != st[:-1]) | (sn[1:] != sn[:-1])
    first = np.flatnonzero(new)
    count = np.diff(np.append(first, n))
    gtags = st[first]
    null_group = (0, 0)
    if nkeys == 1 and first.size and sn[first[-1]] != 0:
        null_group = (int(first[-1]), int(count[-1]))
        gtags, first, count = gtags[:-1], first[:-1], count[:-1]
    assert np.unique(gtags).size == gtags.size, "two different keys share a tag"
    return order, gtags, first.astype(np.uint32), count.astype(np.uint32), null_group


def _key(words, nulls, i):
    return tuple(int(w) for w in words[:, i]), int(nulls[i])


def index_model(words, nulls, order, first, count, null_group=(0, 0)) -> dict:
    """{(words of the key, null bits): (first, count)} from the grouped external rows."""
    words = np.atleast_2d(np.asarray(words, dtype=U64))
    nulls = np.asarray(nulls, dtype=np.uint8)
    model = {}
    groups = list(zip(first.tolist(), count.tolist()))
    if null_group[1]:
        groups.append(null_group)
    for f, c in groups:
        rows = order[f: f + c]
        key = _key(words, nulls, rows[0])
        assert all(_key(words, nulls, r) == key for r in rows), "a group holds two different keys"
        assert key not in model, "one key in two groups"
        model[key] = (int(f), int(c))
    return model


def probe(model, left_words, left_nulls, inner):
    """-> (first int64: grouped position of the first match or -1, count uint32: k for inner and
    max(1, k) for left, keep uint8, total int)."""
    words = np.atleast_2d(np.asarray(left_words, dtype=U64))
    nulls = np.asarray(left_nulls, dtype=np.uint8)
    n = nulls.size
    first = np.full(n, -1, np.int64)
    count = np.zeros(n, np.uint32)
    for i in range(n):
        hit = model.get(_key(words, nulls, i))
        k = 0
        if hit is not None:
            first[i], k = hit
        count[i] = k if inner else max(1, k)
    return first, count, (first >= 0).astype(np.uint8), int(count.astype(U64).sum())


def exclusive_offsets(counts) -> np.ndarray:
    """uint64 exclusive prefix sums, len(counts) entries."""
    c = np.asarray(counts).astype(U64)
    out = np.zeros(c.size, U64)
    if c.size > 1:
        np.cumsum(c[:-1], out=out[1:])
    return out


def expand(offsets, first, m):
    """offsets: n + 1 entries.  -> per output row j < m its left row and its external position
    (first[i] + j - offsets[i], or -1 where first[i] < 0)."""
    off = np.asarray(offsets).astype(np.int64)
    first = np.asarray(first, dtype=np.int64)
    n = first.size
    if m == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    assert off.size == n + 1 and off[n] == m and off[0] == 0
    left = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    f = first[left]
    ext = np.where(f >= 0, f + np.arange(m, dtype=np.int64) - off[left], -1)
    return left, ext


def gather(idx, src, src_valid_bool):
    """-> (values, valid bool): src[idx], 0 and an invalid bit where idx < 0."""
    idx = np.asarray(idx, dtype=np.int64)
    src = np.asarray(src)
    hit = idx >= 0
    vals = np.zeros(idx.size, src.dtype)
    vals[hit] = src[idx[hit]]
    valid = hit.copy()
    if src_valid_bool is not None:
        valid[hit] = np.asarray(src_valid_bool, dtype=bool)[idx[hit]]
    return vals, valid


def surrogate_tags(words, nulls) -> np.ndarray:
    """Tags for the reference pipeline: the word itself for one component; for more, any injective
    numbering of the distinct (words, null bits) tuples (the kernels' fingerprint is internal)."""
    words = np.atleast_2d(np.asarray(words, dtype=U64))
    if words.shape[0] == 1:
        return words[0].copy()
    if words.shape[1] == 0:
        return np.empty(0, U64)
    rows = np.vstack([words, np.asarray(nulls).astype(U64)[None, :]]).T
    return np.unique(rows, axis=0, return_inverse=True)[1].reshape(-1).astype(U64) + U64(1000)


def join_ref(left_keys, ext_keys, modes, inner, payload):
    """The composed reference.  left_keys / ext_keys: one (values, valid bool or None) per component;
    payload: (src, src_valid bool or None) per external column, in external order.

    -> (left_row, ext_row: grouped position or -1, order: external row of a grouped position,
        [(values, valid bool)] per payload column)."""
    nk = len(modes)
    lw, ln = canon_many([k[0] for k in left_keys], [k[1] for k in left_keys], modes)
    ew, en = canon_many([k[0] for k in ext_keys], [k[1] for k in ext_keys], modes)
    order, _, first, count, null_group = group_rows(surrogate_tags(ew, en), en, nk)
    model = index_model(ew, en, order, first, count, null_group)
    f, c, _, total = probe(model, lw, ln, inner)
    off = exclusive_offsets(np.append(c, np.uint32(0)))
    assert int(off[-1]) == total
    left_row, ext_row = expand(off, f, total)
    cols = [gather(ext_row, np.asarray(src)[order], None if v is None else np.asarray(v, dtype=bool)[order])
            for src, v in payload]
    return left_row, ext_row, order, cols


# ---------------------------------------------------------------------------------------------
# a slot table read back
# ---------------------------------------------------------------------------------------------
def check_slots(slots, capacity, empty, group_tags, first, count) -> None:
    """The invariants of a table filled by nvt_join_insert.  ``slots``: capacity x 2 uint64,
    {tag, first | count << 32}.  The order in which lanes win their CAS is not deterministic, so
    positions are not compared:

    * every group tag occurs exactly once, with its {first, count};
    * every other slot is still {empty, 0, 0};
    * every entry is reachable: all slots from home_slot(tag) to its position, cyclically, are
      occupied."""
    slots = np.asarray(slots).view(U64).reshape(-1, 2)
    assert slots.shape[0] == capacity, f"{slots.shape[0]} slots, capacity {capacity}"
    tags, meta = slots[:, 0], slots[:, 1]
    empty = U64(int(empty) & MASK64)
    group_tags = np.asarray(group_tags, dtype=U64)
    want = (np.asarray(first).astype(U64) & U64(0xFFFFFFFF)) | (np.asarray(count).astype(U64) << U64(32))
    assert not (group_tags == empty).any(), "a group tag equals the empty marker"
    occupied = tags != empty
    free_bad = np.flatnonzero(~occupied & (meta != 0))
    assert free_bad.size == 0, f"empty slot {int(free_bad[0])} was overwritten: {int(meta[free_bad[0]]):#x}"
    assert np.unique(group_tags).size == group_tags.size, "the group tags are not distinct"
    pos = np.flatnonzero(occupied)
    by_tag = pos[np.argsort(tags[pos], kind="stable")]
    st = tags[by_tag]
    twice = np.flatnonzero(st[1:] == st[:-1])
    assert twice.size == 0, (f"tag {int(st[twice[0]]):#x} in slots {int(by_tag[twice[0]])} and "
                             f"{int(by_tag[twice[0] + 1])}")
    at = np.searchsorted(st, group_tags)
    found = np.zeros(group_tags.size, bool)
    inside = at < st.size
    found[inside] = st[at[inside]] == group_tags[inside]
    lost = np.flatnonzero(~found)
    assert lost.size == 0, (f"tag {int(group_tags[lost[0]]):#x} of group {int(lost[0])} is not in the table "
                            f"({lost.size} are not)")
    assert st.size == group_tags.size, f"{st.size - group_tags.size} tags in the table belong to no group"
    where = by_tag[at]
    wrong = np.flatnonzero(meta[where] != want)
    assert wrong.size == 0, (f"slot {int(where[wrong[0]])}, tag {int(group_tags[wrong[0]]):#x}: {{first, count}} "
                             f"{int(meta[where[wrong[0]]]):#x}, expected {int(want[wrong[0]]):#x}")
    # run[p]: occupied slots in a row that end at p, cyclically (load <= 0.5: there is an empty slot)
    assert not occupied.all(), "no empty slot"
    idx = np.arange(2 * capacity)
    last_empty = np.maximum.accumulate(np.where(np.tile(occupied, 2), -1, idx))
    run = (idx - last_empty)[capacity:]
    dist = (pos - home_slot(tags[pos], capacity).astype(np.int64)) % capacity
    cut = np.flatnonzero(dist >= run[pos])
    if cut.size:
        p, d = int(pos[cut[0]]), int(dist[cut[0]])
        raise AssertionError(f"tag {int(tags[p]):#x} in slot {p} sits behind the empty slot "
                             f"{(p - int(run[p])) % capacity} (home {(p - d) % capacity})")


def first_mismatch(got, exp, what: str) -> None:
    """assert_array_equal with a message that names the case, the first mismatching row and
    got / expected there."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype, f"{what}: dtype {got.dtype}, expected {exp.dtype}"
    assert got.shape == exp.shape, f"{what}: shape {got.shape}, expected {exp.shape}"
    bad = np.flatnonzero((got != exp).reshape(-1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} elements differ, first at {i}: "
                             f"got {got.reshape(-1)[i]}, expected {exp.reshape(-1)[i]}")
    np.testing.assert_array_equal(got, exp)
