"""Calendar fields of a datetime column: the host driver of nvt_dt_field (include/nvt_hip.h,
csrc/nvt_datetime.hip).  The text side of the type, nvt_csv_parse_datetime, is driven by
kernels_csv.py with the other CSV kernels."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import check

UNIT_CODE = {"s": _lib.DT_S, "ms": _lib.DT_MS, "us": _lib.DT_US, "ns": _lib.DT_NS}
# pandas' names of the fields (Series.dt.<name>), aliases included
FIELD_CODE = {
    "year": _lib.DT_YEAR, "month": _lib.DT_MONTH, "day": _lib.DT_DAY, "hour": _lib.DT_HOUR,
    "minute": _lib.DT_MINUTE, "second": _lib.DT_SECOND,
    "dayofweek": _lib.DT_WEEKDAY, "weekday": _lib.DT_WEEKDAY, "day_of_week": _lib.DT_WEEKDAY,
    "dayofyear": _lib.DT_DAYOFYEAR, "day_of_year": _lib.DT_DAYOFYEAR, "quarter": _lib.DT_QUARTER,
}
UNIT_PER_SECOND = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}


def unit_of(logical) -> str:
    return np.datetime_data(np.dtype(logical))[0]


def dt_field(ts: torch.Tensor, valid: Optional[torch.Tensor], unit: str, field: str) -> torch.Tensor:
    """int32[n]: calendar field ``field`` of the int64 counts ``ts`` in ``unit``; 0 under a
    cleared bit of ``valid``."""
    _lib.require_gpu()
    if ts.dtype != torch.int64 or not ts.is_cuda:
        raise TypeError("dt_field takes int64 counts on the device")
    ts = ts.contiguous()
    n = int(ts.numel())
    out = torch.empty(n, dtype=torch.int32, device=ts.device)
    K.stat_add("dt_field")
    check(_lib.load().nvt_dt_field(ts.data_ptr(), valid.data_ptr() if valid is not None else None, n,
                                   UNIT_CODE[unit], FIELD_CODE[field], out.data_ptr(), K.stream_ptr()), "nvt_dt_field")
    return out
