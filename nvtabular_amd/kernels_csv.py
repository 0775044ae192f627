"""Delimited text -> DeviceFrame: the host driver of the nvt_csv_* entries (include/nvt_hip.h,
csrc/nvt_csv.hip).  One partition's bytes are on the device already; this module indexes the
fields, parses the numeric columns in one launch per 64 of them and the ISO-8601 columns named in
``parse_dates`` in a launch of their own (csrc/nvt_datetime.hip), builds Arrow buffers for the
string columns and keys those as ``kernels_strings.column_from_string_array`` does.

Two read-backs per partition: the field / row counts after the first pass (they size the index
and every output), and the state block with the string columns' char totals after the parse.  A
float field that the device parser declines (more than 19 significant digits, or the one
Eisel-Lemire case 128 bits do not decide) is parsed on the host with ``float()``; only those
fields are read back."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels as K
from . import kernels_strings as KS
from ._lib import check
from .csv_text import DATETIME as _DATETIME   # the dtype of a column named in parse_dates

_TORCH = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}
_CODE = {"int32": _lib.NVT_I32, "int64": _lib.NVT_I64, "float32": _lib.NVT_F32, "float64": _lib.NVT_F64}
_NONE = (1 << 64) - 1


def empty_frame(want, dtypes, device):
    """A partition without rows: the right columns and dtypes, nothing in them."""
    from .device import DeviceColumn, DeviceFrame

    out = {}
    for c in want:
        if dtypes[c] == "string":
            out[c] = DeviceColumn(torch.empty(0, dtype=torch.int64, device=device), None, None, None, {})
        elif dtypes[c] == _DATETIME:
            out[c] = DeviceColumn(torch.empty(0, dtype=torch.int64, device=device), logical=_DATETIME)
        else:
            out[c] = DeviceColumn(torch.empty(0, dtype=_TORCH[dtypes[c]], device=device))
    return DeviceFrame(out)


def _words(n: int, device) -> torch.Tensor:
    """A validity bitmap for n rows: whole 64-bit words, as the kernels store them."""
    return torch.empty(max(1, (n + 63) // 64) * 8, dtype=torch.uint8, device=device)


def index_fields(text: torch.Tensor, nbytes: int, sep: int, quote: int, ncols: int):
    """(field_end, nfields, nrows, state): both passes of the index and the first read-back.
    ``state`` stays on the device; its error words are checked by the caller's later read-back,
    or at once by ``structure_error`` when the counts already disagree."""
    lib = _lib.load()
    dev = text.device
    need = C.c_uint64()
    check(lib.nvt_csv_ws_bytes(nbytes, C.byref(need)), "nvt_csv_ws_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    state = torch.empty(_lib.CSV_STATE_WORDS, dtype=torch.int64, device=dev)
    K.stat_add("csv_index")
    check(lib.nvt_csv_count(text.data_ptr(), nbytes, sep, quote, ws.data_ptr(), need.value, state.data_ptr(),
                            K.stream_ptr()), "nvt_csv_count")
    st = state.cpu().numpy().view(np.uint64)
    nfields, nrows = int(st[_lib.CSV_ST_FIELDS]), int(st[_lib.CSV_ST_ROWS])
    field_end = torch.empty(max(nfields, 1), dtype=torch.int32, device=dev)
    check(lib.nvt_csv_index(text.data_ptr(), nbytes, sep, quote, ncols, ws.data_ptr(), need.value,
                            field_end.data_ptr(), nfields, state.data_ptr(), K.stream_ptr()), "nvt_csv_index")
    return field_end, nfields, nrows, state, int(st[_lib.CSV_ST_PARITY])


def structure_error(st, ncols: int, nrows: int, where: str):
    """The ValueError for a partition whose rows are not ``ncols`` fields each, or None."""
    bad, quote = int(st[_lib.CSV_ST_BAD_ROW]), int(st[_lib.CSV_ST_QUOTE_ROW])
    if quote != _NONE and (bad == _NONE or quote <= bad):
        return ValueError(f"{where}: row {quote}: a newline inside a quoted field (or a quote that is never closed); "
                          f"quoted fields cannot span lines")
    if bad != _NONE:
        return ValueError(f"{where}: row {bad} does not have {ncols} fields (rows are not padded or truncated)")
    if int(st[_lib.CSV_ST_PARITY]):
        return ValueError(f"{where}: row {nrows}: a quote that is never closed")
    return None


def _field_error(code: int, names, dtypes, where: str, text: str = None):
    row, k, rc = code >> 24, (code >> 2) & ((1 << 22) - 1), code & 3
    name = names[k]
    if dtypes[name] == "string":
        what = "has a quote inside its quotes that is not doubled"
    elif dtypes[name] == _DATETIME:
        what = ("lies outside the range of datetime64[ns] (1677-09-21 to 2262-04-11)" if rc == _lib.CSV_OVERFLOW
                else "is not YYYY-MM-DD[(T| )HH:MM[:SS[.fffffffff]]] (no zone, no blanks) or names no calendar day")
        shown = f" {text!r}" if text is not None else ""
        return ValueError(f"{where}: row {row}, column '{name}': the field{shown} {what}; "
                          f"leave '{name}' out of parse_dates to read the column as text")
    else:
        what = f"does not fit {dtypes[name]}" if rc == _lib.CSV_OVERFLOW else f"does not parse as {dtypes[name]}"
    shown = f" {text!r}" if text is not None else ""
    return ValueError(f"{where}: row {row}, column '{name}': the field{shown} {what}; "
                      f"pass dtypes={{'{name}': ...}} to read the column as another type")


def _host_fields(rows: torch.Tensor, k: int, ncols: int, field_end: torch.Tensor, host: np.ndarray, quote: int):
    """The text of field k of the given rows, read from the host copy of the partition."""
    f = rows * ncols + k
    ends = field_end[f].cpu().numpy()
    prev = field_end[torch.clamp(f - 1, min=0)].cpu().numpy()
    starts = np.where(f.cpu().numpy() > 0, prev + 1, 0)   # (field 0 of row 0 starts the text)
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        raw = host[s:e].tobytes()
        if k == ncols - 1 and raw.endswith(b"\r"):
            raw = raw[:-1]
        if quote >= 0 and len(raw) >= 2 and raw[0] == quote and raw[-1] == quote:
            raw = raw[1:-1]
        out.append(raw)
    return out


def parse_text(text: torch.Tensor, nbytes: int, host: np.ndarray, sep: int, quote: int, names, dtypes, want,
               where: str):
    """One partition -> DeviceFrame with the columns ``want``.  ``text``: the bytes on the device
    (16-byte aligned, readable to a multiple of 16), ``host``: the same bytes on the host."""
    from .device import DeviceColumn, DeviceFrame

    lib = _lib.load()
    dev = text.device
    ncols = len(names)
    s = K.stream_ptr()
    field_end, nfields, nrows, state, parity = index_fields(text, nbytes, sep, quote, ncols)
    if parity or nfields != nrows * ncols:
        st = state.cpu().numpy().view(np.uint64)
        raise structure_error(st, ncols, nrows, where) or ValueError(f"{where}: malformed text")
    if nrows == 0:
        return empty_frame(want, dtypes, dev)
    n = nrows
    numeric = [c for c in want if dtypes[c] not in ("string", _DATETIME)]
    dates = [c for c in want if dtypes[c] == _DATETIME]
    strings = [c for c in want if dtypes[c] == "string"]
    data, valid, slow = {}, {}, {}
    if numeric:
        descs = (_lib.CsvCol * len(numeric))()
        for d, c in zip(descs, numeric):
            data[c] = torch.empty(n, dtype=_TORCH[dtypes[c]], device=dev)
            valid[c] = _words(n, dev)
            d.out, d.out_valid, d.k, d.dtype = data[c].data_ptr(), valid[c].data_ptr(), names.index(c), _CODE[dtypes[c]]
            if dtypes[c].startswith("float"):
                slow[c] = _words(n, dev)
                d.slow = slow[c].data_ptr()
        K.stat_add("csv_parse_many")
        check(lib.nvt_csv_parse_many(text.data_ptr(), nbytes, field_end.data_ptr(), n, ncols, quote, descs,
                                     len(numeric), state.data_ptr(), s), "nvt_csv_parse_many")
    if dates:
        # a kernel of its own behind the numeric one (the float parser sets that one's registers)
        descs = (_lib.CsvCol * len(dates))()
        for d, c in zip(descs, dates):
            data[c] = torch.empty(n, dtype=torch.int64, device=dev)
            valid[c] = _words(n, dev)
            d.out, d.out_valid, d.k, d.dtype = data[c].data_ptr(), valid[c].data_ptr(), names.index(c), _lib.NVT_I64
        K.stat_add("csv_parse_datetime")
        check(lib.nvt_csv_parse_datetime(text.data_ptr(), nbytes, field_end.data_ptr(), n, ncols, quote, descs,
                                         len(dates), state.data_ptr(), s), "nvt_csv_parse_datetime")
    offsets = {}
    if strings:
        need = C.c_uint64()
        check(lib.nvt_csv_str_ws_bytes(n, C.byref(need)), "nvt_csv_str_ws_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        for c in strings:
            offsets[c] = torch.empty(n + 1, dtype=torch.int32, device=dev)
            valid[c] = _words(n, dev)
            K.stat_add("csv_str_offsets")
            check(lib.nvt_csv_str_offsets(text.data_ptr(), nbytes, field_end.data_ptr(), n, ncols, names.index(c),
                                          quote, offsets[c].data_ptr(), valid[c].data_ptr(), ws.data_ptr(),
                                          need.value, state.data_ptr(), s), "nvt_csv_str_offsets")
    # the second read-back: error words, the slow-path count and the char total of every string column
    tail = [state] + [offsets[c][n:].to(torch.int64) for c in strings]
    st = torch.cat(tail).cpu().numpy().view(np.uint64)
    err = structure_error(st, ncols, nrows, where)
    if err is not None:
        raise err
    if int(st[_lib.CSV_ST_BAD_FIELD]) != _NONE:
        code = int(st[_lib.CSV_ST_BAD_FIELD])
        row = torch.tensor([code >> 24], dtype=torch.int64, device=dev)
        shown = _host_fields(row, (code >> 2) & ((1 << 22) - 1), ncols, field_end, host, quote)[0]
        raise _field_error(code, names, dtypes, where, shown.decode("utf-8", "replace"))
    K.stat_add("csv_float_fields", n * len(slow))     # (tools/csv_rate.py reports the share)
    K.stat_add("csv_slow_fields", int(st[_lib.CSV_ST_SLOW]))
    if int(st[_lib.CSV_ST_SLOW]):
        for c, bm in slow.items():
            rows = K.unpack_bitmap(bm, n).nonzero().reshape(-1)
            if rows.numel() == 0:
                continue
            k = names.index(c)
            vals = []
            for r, raw in zip(rows.cpu().tolist(), _host_fields(rows, k, ncols, field_end, host, quote)):
                try:
                    vals.append(float(raw.decode("ascii")))
                except (ValueError, UnicodeDecodeError):
                    raise _field_error((r << 24) | (k << 2) | _lib.CSV_INVALID, names, dtypes, where,
                                       raw.decode("utf-8", "replace")) from None
            data[c][rows] = torch.tensor(vals, dtype=torch.float64).to(data[c].dtype).to(dev)
    out = {}
    for i, c in enumerate(strings):
        total = int(st[_lib.CSV_STATE_WORDS + i])
        chars = torch.empty(max(8, (total + 7) & ~7), dtype=torch.uint8, device=dev)
        K.stat_add("csv_str_copy")
        check(lib.nvt_csv_str_copy(text.data_ptr(), nbytes, field_end.data_ptr(), n, ncols, names.index(c), quote,
                                   offsets[c].data_ptr(), chars.data_ptr(), total, s), "nvt_csv_str_copy")
        b = KS.StringBuffers(n, offsets[c], 4, chars, total, valid[c])
        keys = KS.hash_buffers(b)
        out[c] = DeviceColumn(keys, valid[c], None, None, KS.lookup_dict(keys, valid[c], b))
    for c in numeric:
        out[c] = DeviceColumn(data[c], valid[c])
    for c in dates:
        out[c] = DeviceColumn(data[c], valid[c], logical=_DATETIME)
    return DeviceFrame({c: out[c] for c in want})
