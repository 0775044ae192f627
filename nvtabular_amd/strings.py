"""Front-end for string categoricals.

The hot path (Criteo) is integer ids; string columns are supported by mapping
every string to a 64-bit surrogate key (pandas' keyed siphash,
``pandas.util.hash_array`` -- the primitive the reference's pandas-backed
``hash_series`` builds on) and letting the HIP kernels count / encode the
surrogates.  The column remembers {surrogate -> string} so vocabularies can be
written with the original values and ordered by them.

Columns that Arrow holds as ``string`` / ``large_string`` are keyed on the device
from their Arrow buffers (``kernels_strings``: the same bits); ``string_key64`` /
``string_column_to_device`` below are the host path, kept as the exact fall-back
for values Arrow does not type as strings (bytes, mixed types, text that does not
encode as UTF-8).
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch


def string_key64(values) -> np.ndarray:
    arr = np.asarray(values, dtype=object)
    return pd.util.hash_array(arr, categorize=False).view(np.int64)


def string_column_to_device(s: pd.Series, device):
    from .device import DeviceColumn, pack_bitmap

    mask = s.isna().to_numpy()
    vals = s.to_numpy(dtype=object)
    keys = np.zeros(len(s), dtype=np.int64)
    lut = {}
    if (~mask).any():
        uniq = pd.unique(vals[~mask])
        ukeys = string_key64(uniq)
        lut = dict(zip(ukeys.tolist(), uniq.tolist()))
        if len(lut) != len(uniq):
            raise ValueError("64-bit surrogate collision between distinct strings")
        keys[~mask] = string_key64(vals[~mask])
    data = torch.from_numpy(keys).to(device)
    valid = torch.from_numpy(pack_bitmap(~mask)).to(device) if mask.any() else None
    return DeviceColumn(data, valid, None, None, lut)


def as_string_array(s: pd.Series):
    """The Series as a pyarrow string / large_string array, or None when pyarrow types it
    otherwise (bytes -> binary, all missing -> null) or rejects it (mixed types, text that does
    not encode as UTF-8): those take the host path."""
    import pyarrow as pa

    from .kernels_strings import fits, is_string_type

    try:
        arr = pa.array(s, from_pandas=True)
    except (pa.ArrowException, UnicodeError, TypeError, ValueError):
        return None
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    if not is_string_type(arr.type) or not fits(arr):
        return None
    return arr


def string_series_to_device(s: pd.Series, device):
    """A string Series -> DeviceColumn, on the device when Arrow types it as strings."""
    from .kernels_strings import column_from_string_array

    arr = as_string_array(s)
    if arr is None:
        return string_column_to_device(s, device)
    return column_from_string_array(arr, device)


def string_keys(s: pd.Series, device) -> torch.Tensor:
    """int64 surrogate of every row of a string Series (0 for a missing value) on ``device`` --
    vocabulary and statistics files read back for a transform."""
    from .kernels_strings import hash_array

    arr = as_string_array(s)
    if arr is not None:
        return hash_array(arr, device)
    mask = s.isna().to_numpy()
    keys = np.zeros(len(s), dtype=np.int64)
    if (~mask).any():
        keys[~mask] = string_key64(s.to_numpy(dtype=object)[~mask])
    return torch.from_numpy(keys).to(device)
