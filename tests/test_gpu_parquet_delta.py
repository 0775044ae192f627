"""pyarrow-written DELTA_BINARY_PACKED files through ``nvt.Dataset`` on the device equal ``pq.read_table``,
and no chunk goes to pyarrow's reader (without delta pages in the reader the whole file does)."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import nvtabular_amd as nvt
from nvtabular_amd import parquet_plain as PP
from test_parquet_delta_host import mixed_chunk

pytestmark = pytest.mark.gpu

ROWS = 6000
DELTA = ["id", "i32n", "i16n", "ts"]


def _table():
    rng = np.random.default_rng(11)

    def nulls(v, typ):
        return pa.array(v, type=typ, mask=rng.random(ROWS) < 0.3)

    fields = [pa.field("id", pa.int64(), nullable=False), pa.field("i32n", pa.int32()), pa.field("i16n", pa.int16()),
              pa.field("ts", pa.timestamp("ns")), pa.field("f32", pa.float32()), pa.field("cat", pa.int64())]
    ts = np.int64(1_700_000_000_000_000_000) + np.cumsum(rng.integers(0, 10**9, ROWS))
    arrays = [pa.array(np.cumsum(rng.integers(1, 50, ROWS)) + 10**12),
              nulls(rng.integers(-2**31, 2**31, ROWS).astype(np.int32), pa.int32()),
              nulls(rng.integers(-2**15, 2**15, ROWS).astype(np.int16), pa.int16()),
              pa.array(ts, type=pa.timestamp("ns")),
              pa.array(rng.random(ROWS).astype(np.float32)),
              pa.array(rng.integers(0, 40, ROWS) * 10**10)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_dataset_reads_delta_files_on_the_device(tmp_path, version, compression):
    path = str(tmp_path / "delta.parquet")
    pq.write_table(_table(), path, column_encoding={c: "DELTA_BINARY_PACKED" for c in DELTA}, use_dictionary=["cat"],
                   data_page_version=version, compression=compression, data_page_size=4096, row_group_size=ROWS // 2)
    assert pq.read_metadata(path).num_row_groups == 2 and PP.PlainParquetFile(path).decodable
    exp = pq.read_table(path)
    before = dict(PP.READER_CHUNKS)
    frames = list(nvt.Dataset(path, engine="parquet").to_iter())
    assert PP.READER_CHUNKS["pyarrow"] == before["pyarrow"]
    assert PP.READER_CHUNKS["plain"] - before["plain"] == 2 * exp.num_columns
    got = pa.concat_tables([f.to_arrow() for f in frames])
    assert got.column_names == exp.column_names
    for c in exp.column_names:
        assert got.column(c).combine_chunks().equals(exp.column(c).combine_chunks()), c
    df = nvt.Dataset(path, engine="parquet").compute()
    np.testing.assert_array_equal(df["id"].to_numpy(), exp.column("id").to_numpy())


def test_plain_and_delta_pages_of_one_chunk_meet_on_the_device():
    """Only the host-decoded runs between the holes are copied (``values_to_device``); the holes are filled."""
    x, (rc, msg, stage, vals) = mixed_chunk()
    assert rc == 0, msg
    sc = PP.StagedColumn(vals, None, len(x), len(x), np.dtype("int64"))
    sc.delta = stage
    frame = PP.StagedPartition({"x": sc}).to_device(torch.device("cuda:0"))
    np.testing.assert_array_equal(frame["x"].data.cpu().numpy(), x)
