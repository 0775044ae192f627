"""Snappy PLAIN pages through the device route: ``read_row_groups_staged(device_inflate=True)`` +
``to_device`` and ``nvt.Dataset`` with ``io.PQ_DEVICE_INFLATE`` equal ``pq.read_table`` bit for bit, and
``READER_CHUNKS["inflate_pages"]`` grows by the eligible pages counted from the page headers."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import inflate_reference as IR
import nvtabular_amd as nvt
from nvtabular_amd import io as nvt_io
from nvtabular_amd import kernels as K
from nvtabular_amd import parquet_plain as PP
from test_gpu_parquet_dict_in import _same   # (validity, then the values bit for bit)

pytestmark = pytest.mark.gpu


def _both_ways(path, monkeypatch, exp=None, routed=True):
    """Staged read + to_device, then Dataset with the switch on; each must count the eligible pages."""
    exp = pq.read_table(path) if exp is None else exp
    eligible = sum(IR.eligible_pages(path).values())
    assert (eligible > 0) == routed
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    before, launches = PP.READER_CHUNKS["inflate_pages"], K.STATS.get("pq_inflate", 0)
    staged = PP.read_row_groups_staged(pf, list(range(pf.num_row_groups)), device_inflate=True)
    _same(PP.StagedPartition(staged).to_device().to_arrow(), exp)
    assert PP.READER_CHUNKS["inflate_pages"] - before == eligible
    assert (K.STATS.get("pq_inflate", 0) - launches == 1) == routed   # one launch for the partition
    monkeypatch.setattr(nvt_io, "PQ_DEVICE_INFLATE", True)
    before, pyarrow_chunks = PP.READER_CHUNKS["inflate_pages"], PP.READER_CHUNKS["pyarrow"]
    frames = list(nvt.Dataset(path, engine="parquet").to_iter())
    _same(pa.concat_tables([f.to_arrow() for f in frames]), exp)
    assert PP.READER_CHUNKS["inflate_pages"] - before == eligible and PP.READER_CHUNKS["pyarrow"] == pyarrow_chunks


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_number_columns_several_pages_two_row_groups(tmp_path, monkeypatch, version, nullable):
    path = str(tmp_path / "z.parquet")
    _both_ways(path, monkeypatch, IR.write(path, version, nullable))


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_one_large_page(tmp_path, monkeypatch, version):
    path = str(tmp_path / "one.parquet")
    t = IR.table(30_000, True).select(["i64"])
    pq.write_table(t, path, compression="snappy", use_dictionary=False, data_page_size=1 << 20,
                   data_page_version=version)
    assert IR.eligible_pages(path)["i64"] in (1, 2)   # (pyarrow ends a page at 20 000 rows: 160 000 bytes)
    _both_ways(path, monkeypatch)


def test_a_column_with_nulls_stays_on_the_host(tmp_path, monkeypatch):
    path = str(tmp_path / "n.parquet")
    exp = IR.write(path, "1.0", True, with_nulls=("f64",), row_group_size=5000)
    assert exp.column("f64").null_count > 0
    eligible = IR.eligible_pages(path)
    assert eligible["f64"] == 0 and min(eligible[c] for c in ("i32", "i64", "ts")) > 1
    _both_ways(path, monkeypatch, exp)


def test_pyarrow_default_chunk_falls_back_to_plain_half_way(tmp_path, monkeypatch):
    path = str(tmp_path / "d.parquet")
    ids = np.random.default_rng(5).permutation(20_000).astype(np.int64) * 977
    pq.write_table(pa.table({"id": ids, "small": (ids % 7).astype(np.int32)}), path, dictionary_pagesize_limit=4096,
                   data_page_size=8192)
    md = pq.read_metadata(path).row_group(0).column(0)
    assert md.has_dictionary_page and "PLAIN" in md.encodings and "RLE_DICTIONARY" in md.encodings
    assert IR.eligible_pages(path)["small"] == 0
    _both_ways(path, monkeypatch)


def test_files_of_the_device_snappy_writer(tmp_path, monkeypatch):
    t = IR.table(5000, False)
    nvt.Dataset(t.to_pandas()).to_parquet(str(tmp_path / "w"), device_compression="snappy")
    files = sorted(str(p) for p in (tmp_path / "w").glob("*.parquet"))
    assert files
    for f in files:
        _both_ways(f, monkeypatch)   # (asserts that pages took the route)


def test_uncompressed_file_is_untouched(tmp_path, monkeypatch):
    path = str(tmp_path / "u.parquet")
    _both_ways(path, monkeypatch, IR.write(path, "1.0", True, compression="none"), routed=False)
