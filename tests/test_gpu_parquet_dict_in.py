"""pyarrow's default files (every flat column dictionary-encoded) through ``nvt.Dataset``: the dictionary
pages of number columns are filled on the device (the ``pq_dict_fill`` launch counter moves) and the
frames equal ``pq.read_table``, as they do with the host route (``io.PQ_DEVICE_DICT = False``)."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import dict_in_reference as DI
import nvtabular_amd as nvt
from nvtabular_amd import io as nvt_io
from nvtabular_amd import kernels as K
from nvtabular_amd import parquet_plain as PP

pytestmark = pytest.mark.gpu


def _read(path, **kw):
    frames = list(nvt.Dataset(path, engine="parquet", **kw).to_iter())
    return pa.concat_tables([f.to_arrow() for f in frames])


def _same(got, exp):
    assert got.column_names == exp.column_names and got.num_rows == exp.num_rows
    for c in exp.column_names:   # validity, then the values as integers: NaNs bit for bit
        a, b = got.column(c).combine_chunks(), exp.column(c).combine_chunks()
        assert a.type == b.type, c
        np.testing.assert_array_equal(np.asarray(a.is_valid()), np.asarray(b.is_valid()), err_msg=c)
        a, b = (x.cast(pa.int64()) if pa.types.is_timestamp(x.type) else x for x in (a, b))
        a, b = (x.fill_null(0).to_numpy(zero_copy_only=False) for x in (a, b))
        np.testing.assert_array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}"), err_msg=c)


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("nullable", [False, True])
def test_dataset_fills_dictionary_pages_on_the_device(tmp_path, monkeypatch, nullable, version, compression):
    path = str(tmp_path / "d.parquet")
    exp = DI.write(path, nullable, compression, version)
    monkeypatch.setattr(nvt_io, "PQ_DEVICE_DICT", True)
    chunks, fills = dict(PP.READER_CHUNKS), K.STATS.get("pq_dict_fill", 0)
    _same(_read(path), exp)
    assert PP.READER_CHUNKS["pyarrow"] == chunks["pyarrow"]
    assert K.STATS.get("pq_dict_fill", 0) > fills
    df, want = nvt.Dataset(path, engine="parquet").compute(), exp.to_pandas()
    for c in ("i64", "f64", "wide"):   # (nulls are NaN / NA in a pandas frame: compared as float64)
        np.testing.assert_array_equal(df[c].to_numpy(dtype="float64", na_value=np.nan),
                                      want[c].to_numpy(dtype="float64", na_value=np.nan), err_msg=c)
    fills = K.STATS.get("pq_dict_fill", 0)
    monkeypatch.setattr(nvt_io, "PQ_DEVICE_DICT", False)
    _same(_read(path), exp)
    assert K.STATS.get("pq_dict_fill", 0) == fills


def test_filters_on_a_dictionary_column(tmp_path, monkeypatch):
    path = str(tmp_path / "f.parquet")
    DI.write(path, True, "snappy", "1.0")
    monkeypatch.setattr(nvt_io, "PQ_DEVICE_DICT", True)
    filters = [("i8", ">", 3), ("f64", "<", 0.5)]
    fills = K.STATS.get("pq_dict_fill", 0)
    _same(_read(path, filters=filters), pq.read_table(path, filters=filters))
    assert K.STATS.get("pq_dict_fill", 0) > fills
