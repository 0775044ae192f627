"""Parquet string columns through the hand-written reader on the GPU: every partition equals the one
the pyarrow path builds (keys, validity, dict, pandas frame), the reader counts its chunks, a
workflow on the file equals the workflow on the pandas frame, and an index past its dictionary is
reported, not followed."""
import glob
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import pq_str_files as F
from nvtabular_amd.parquet_thrift import _TReader

pytestmark = pytest.mark.gpu


def _parts(path, plain, rgpp, monkeypatch, columns=None):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio

    monkeypatch.setattr(nio, "PLAIN_PARQUET_READ", plain)
    ds = nvt.Dataset(path, engine="parquet", row_groups_per_part=rgpp)
    return [f for f in ds.to_iter(columns=columns)] if columns else [f for f in ds.to_iter()]


@pytest.mark.parametrize("rgpp", [1, 2])
@pytest.mark.parametrize("name", sorted(F.CASES))
def test_partitions_equal_the_pyarrow_path(tmp_path, name, rgpp, monkeypatch):
    from nvtabular_amd.parquet_plain import READER_CHUNKS

    path = str(tmp_path / f"{name}.parquet")
    t = F.write(name, path)
    md = pq.ParquetFile(path).metadata
    before = dict(READER_CHUNKS)
    a = _parts(path, True, rgpp, monkeypatch)
    # with the reader on nothing goes to pyarrow, and every column chunk is counted
    assert READER_CHUNKS["pyarrow"] == before["pyarrow"]
    assert READER_CHUNKS["plain"] - before["plain"] == t.num_columns * md.num_row_groups
    b = _parts(path, False, rgpp, monkeypatch)
    assert len(a) == len(b) == -(-md.num_row_groups // rgpp) and sum(len(f) for f in a) == t.num_rows
    for fa, fb in zip(a, b):
        assert list(fa.columns) == list(fb.columns) and len(fa) == len(fb)
        ca, cb = fa["s"], fb["s"]
        assert ca.data.dtype == cb.data.dtype == torch.int64
        assert torch.equal(ca.data, cb.data)
        ma, mb = ca.valid_mask_host(), cb.valid_mask_host()
        assert (ma is None) == (mb is None) and (ca.valid is None) == (cb.valid is None)
        if ma is not None:
            np.testing.assert_array_equal(ma, mb)
            assert not ca.data.cpu().numpy()[~ma].any()            # key 0 under a null
        assert list(ca.strings.items()) == list(cb.strings.items())
        pd.testing.assert_frame_equal(fa.to_pandas(), fb.to_pandas())
    got = pd.concat([f.to_pandas() for f in a], ignore_index=True)["s"]
    want = t["s"].to_pandas()
    assert [None if pd.isna(v) else v for v in got] == [None if pd.isna(v) else v for v in want]


def test_projection_reads_only_the_string_column(tmp_path, monkeypatch):
    from nvtabular_amd.parquet_plain import READER_CHUNKS

    path = str(tmp_path / "p.parquet")
    t = F.write("small_dict_v2", path)
    before = dict(READER_CHUNKS)
    parts = _parts(path, True, 2, monkeypatch, columns=["s"])
    assert READER_CHUNKS["plain"] - before["plain"] == pq.ParquetFile(path).num_row_groups
    assert READER_CHUNKS["pyarrow"] == before["pyarrow"]
    assert all(list(f.columns) == ["s"] for f in parts)
    got = pd.concat([f.to_pandas() for f in parts], ignore_index=True)["s"]
    assert [None if pd.isna(v) else v for v in got] == t["s"].to_pylist()


def test_workflow_on_the_file_equals_the_workflow_on_the_frame(tmp_path, monkeypatch):
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd import ops
    from nvtabular_amd.parquet_plain import READER_CHUNKS

    monkeypatch.setattr(nio, "PLAIN_PARQUET_READ", True)
    path = str(tmp_path / "w.parquet")
    t = F.write("default", path)

    def run(source, tag, **kw):
        cat = ["s"] >> ops.Categorify(out_path=str(tmp_path / tag))
        cont = ["f"] >> ops.FillMissing() >> ops.Normalize()
        out = nvt.Workflow(cat + cont).fit_transform(nvt.Dataset(source, **kw)).to_ddf().compute()
        (uniq,) = glob.glob(os.path.join(str(tmp_path / tag), "**", "unique.s.parquet"), recursive=True)
        return out, pd.read_parquet(uniq)

    before = dict(READER_CHUNKS)
    got, got_uniq = run(path, "file", engine="parquet")
    assert READER_CHUNKS["pyarrow"] == before["pyarrow"] and READER_CHUNKS["plain"] > before["plain"]
    want, want_uniq = run(t.to_pandas(), "frame")
    np.testing.assert_array_equal(got["s"].to_numpy(), want["s"].to_numpy())
    np.testing.assert_array_equal(got["f"].to_numpy(), want["f"].to_numpy())
    pd.testing.assert_frame_equal(got_uniq, want_uniq)


def test_an_index_past_the_dictionary_raises(tmp_path, monkeypatch):
    """The first bit-packed index of an uncompressed v1 page is patched to 7 in a file whose
    dictionary holds 5 entries: every read of the run stays inside the staged bytes, the id fails the
    range check on the device, and the error names file and column."""
    import nvtabular_amd as nvt
    from nvtabular_amd import io as nio
    from nvtabular_amd.parquet_plain import PlainParquetFile

    monkeypatch.setattr(nio, "PLAIN_PARQUET_READ", True)
    words = ["a", "bb", "ccc", "dddd", "eeeee"]
    vals = [words[i % 5] for i in range(1000)]
    path = str(tmp_path / "bad.parquet")
    schema = pa.schema([pa.field("s", pa.string(), nullable=False)])
    pq.write_table(pa.table({"s": pa.array(vals)}, schema=schema), path, compression=None, data_page_version="1.0",
                   write_page_checksum=False)
    data = bytearray(open(path, "rb").read())
    at = PlainParquetFile(path).row_groups[0]["columns"][0]["offset"]
    r = _TReader(data, at)
    head = r.struct()
    assert head[1] == 2                                   # the dictionary page
    r.p += head[3]
    head = r.struct()
    assert head[1] == 0 and head[5][2] in (2, 8)          # a v1 data page of dictionary indices
    body = r.p
    assert data[body] == 3 and data[body + 1] & 1         # bit width 3, a bit-packed run first
    data[body + 2] |= 0x07                                # its first index: 7
    open(path, "wb").write(bytes(data))
    ds = nvt.Dataset(path, engine="parquet")
    with pytest.raises(ValueError, match=r"bad\.parquet.*'s'.*1 dictionary ind"):
        list(ds.to_iter())
    torch.cuda.synchronize()                              # nothing faulted
