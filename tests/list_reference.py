"""Plain Python / numpy statements of what the session kernels of nvt_list.hip compute (ListSlice,
ValueCount, DifferenceLag), as include/nvt_hip.h words them.  Nothing here imports the package:
test_list_reference.py pins these functions to independent formulations on the CPU and
test_gpu_list_kernels.py compares the kernels with them bit for bit.

A list column is its leaves plus n + 1 int64 row offsets; offsets[0] may be non-zero, leaf 0 of the
values is the leaf offsets[0] names.  Validity travels as a bool array per leaf (None = all valid);
``pack_bits`` turns it into the bitmap bytes the kernels read and write (LSB first, padded with
zero bits to whole 64-bit words)."""
import numpy as np

INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)


def pack_bits(ok):
    """bool[m] -> uint8[ceil(m / 64) * 8], bit i of byte i // 8 = ok[i], the bits past m zero."""
    ok = np.asarray(ok, dtype=bool)
    out = np.zeros((len(ok) + 63) // 64 * 8, dtype=np.uint8)
    packed = np.packbits(ok, bitorder="little")
    out[: len(packed)] = packed
    return out


def sliced_len(L, start, end):
    """len(row[start:end]) of a row of L leaves, without the row: Python slices a range object of
    any length exactly, so rows of 2^40 leaves cost nothing."""
    return len(range(int(L))[int(start): int(end)])


def slice_offsets(off, start, end):
    """The n + 1 new offsets (from 0) of row[start:end] for every row."""
    off = [int(v) for v in off]
    out = np.zeros(len(off), dtype=np.int64)
    run, seen = 0, {}
    for i in range(len(off) - 1):
        L = off[i + 1] - off[i]
        if L not in seen:
            seen[L] = sliced_len(L, start, end)
        run += seen[L]
        out[i + 1] = run
    return out


def slice_rows(vals, valid, off, start, end, pad_width=None, pad_value=0):
    """(leaves, leaf validity bool[], new offsets): row i = row[start:end]; with ``pad_width`` every
    row is then filled up to that many leaves with ``pad_value`` cast to the leaf dtype, the padded
    leaves valid.  The operator never asks for a width below a sliced row, and neither may a caller
    of this function."""
    vals = np.asarray(vals)
    o0 = int(off[0])
    out_v, out_ok, new_off = [], [], np.zeros(len(off), dtype=np.int64)
    pad = np.array([pad_value]).astype(vals.dtype)
    for i in range(len(off) - 1):
        a, b = int(off[i]) - o0, int(off[i + 1]) - o0
        row = vals[a:b][int(start): int(end)]
        ok = (np.ones(b - a, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)[a:b])[int(start): int(end)]
        if pad_width is not None:
            k = pad_width - len(row)
            assert k >= 0, "pad_width below a sliced row"
            row = np.concatenate([row, np.repeat(pad, k)])
            ok = np.concatenate([ok, np.ones(k, dtype=bool)])
        out_v.append(row)
        out_ok.append(ok)
        new_off[i + 1] = new_off[i] + len(row)
    cat = np.concatenate(out_v).astype(vals.dtype) if out_v else vals[:0]
    return cat, (np.concatenate(out_ok) if out_ok else np.zeros(0, dtype=bool)), new_off


def len_minmax(off):
    """(min, max) of offsets[i + 1] - offsets[i] as Python ints; n = 0 leaves the accumulator's
    start values."""
    d = [int(off[i + 1]) - int(off[i]) for i in range(len(off) - 1)]
    return (min(d), max(d)) if d else (INT64_MAX, INT64_MIN)


def lag(keys, x, valid, shift):
    """float32[n]: out[i] = x[i] - x[j], j = i - shift, where 0 <= j < n, every partition column
    of ``keys`` ([(values, validity bool[] or None)]) is non-null and equal at i and j (NaN equals
    nothing, itself included) and x is valid at both; NaN elsewhere.  Integers are converted to
    float64 before the subtraction, float64 subtracts in float64, float32 in float32; the
    difference is rounded to float32."""
    x = np.asarray(x)
    n, shift = len(x), int(shift)
    out = np.full(n, np.nan, dtype=np.float32)
    if abs(shift) >= n:
        return out
    i = np.arange(max(shift, 0), n + min(shift, 0))
    j = i - shift
    ok = np.ones(len(i), dtype=bool)
    for k, kv in keys:
        k = np.asarray(k)
        if kv is not None:
            ok &= np.asarray(kv, dtype=bool)[i] & np.asarray(kv, dtype=bool)[j]
        ok &= k[i] == k[j]
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool)[i] & np.asarray(valid, dtype=bool)[j]
    with np.errstate(all="ignore"):
        if x.dtype == np.float32:
            d = x[i] - x[j]
        elif x.dtype == np.float64:
            d = (x[i] - x[j]).astype(np.float32)
        else:
            d = (x[i].astype(np.float64) - x[j].astype(np.float64)).astype(np.float32)
    out[i[ok]] = d[ok]
    return out
