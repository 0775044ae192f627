"""DELTA_BINARY_PACKED in the parquet reader, host half: the verdict on pyarrow's delta files, what is staged
for the device (decoded here with tests/delta_reference.py), mixed chunks, corrupt pages: errors."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import delta_reference as DR
from nvtabular_amd import _lib
from nvtabular_amd import kernels_parquet_delta as KPD
from nvtabular_amd import parquet_plain as PP

ROWS = 5000
W = _lib.PQ_DELTA_RECORD_WORDS   # words of a staged page record


def _column(kind, nullable):
    rng = np.random.default_rng(3)
    if kind == "int32":
        arr = pa.array(rng.integers(-2**31, 2**31, ROWS).astype(np.int32))
    else:
        arr = pa.array(np.cumsum(rng.integers(0, 1 << 40, ROWS)) - (1 << 50))
        arr = arr.cast(pa.timestamp("us")) if kind == "timestamp" else arr
    if nullable:
        arr = pa.array(arr.to_pylist(), type=arr.type, mask=rng.random(ROWS) < 0.3)
    return pa.Table.from_arrays([arr], schema=pa.schema([pa.field("x", arr.type, nullable=nullable)]))


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("kind", ["int32", "int64", "timestamp"])
def test_pyarrow_delta_chunks_are_staged_for_the_device(tmp_path, kind, nullable, version, compression):
    table = _column(kind, nullable)
    path = str(tmp_path / "d.parquet")
    pq.write_table(table, path, column_encoding={"x": "DELTA_BINARY_PACKED"}, use_dictionary=False,
                   data_page_version=version, compression=compression, data_page_size=4096, row_group_size=3000)
    pf = PP.PlainParquetFile(path)
    assert pf.decodable, pf.why_pyarrow
    assert not pf.eligible and not pf.readable and "DELTA_BINARY_PACKED" in pf.why
    before = PP.READER_CHUNKS["plain"]
    sc = PP.read_row_groups_staged(pf, [0, 1], pin=False)["x"]
    assert PP.READER_CHUNKS["plain"] - before == 2
    col = table.column("x").combine_chunks()
    mask = np.asarray(col.is_valid())
    assert sc.rows == ROWS and sc.nvalid == int(mask.sum())
    if nullable:
        np.testing.assert_array_equal(np.unpackbits(sc.valid.numpy(), bitorder="little")[:ROWS].astype(bool), mask)
    else:
        assert sc.valid is None
    bits = 32 if kind == "int32" else 64
    vals = sc.values[:sc.nvalid].numpy().copy()
    vals[:] = -7   # (every value must come out of a staged page)
    first, pos, count, vpm, _ = KPD.page_records(sc.delta)
    at = sc.delta.pages[: W * sc.delta.npages].numpy().reshape(-1, W)[:, 4]
    assert sc.delta.npages > 2 and int(count.sum()) == sc.nvalid and set(vpm.tolist()) <= {32, 64}
    staged = sc.delta.bytes.numpy()
    for p in range(sc.delta.npages):
        got = DR.decode(staged[int(at[p]): sc.delta.nbytes], bits)
        assert len(got) == int(count[p]) and got[0] == np.int64(first[p].astype(np.int64))
        vals[int(pos[p]): int(pos[p]) + len(got)] = got
    want = col.drop_null()
    want = (want.cast(pa.int64()) if kind == "timestamp" else want).to_numpy()
    np.testing.assert_array_equal(vals, want)
    assert sc.logical == (np.dtype("datetime64[us]") if kind == "timestamp" else None)


def _decode_chunk(pages, ptype=1):
    """A chunk of v1 pages [(encoding, region, values)], required column -> (rc, message, stage, packed values)."""
    lib = _lib.load()
    chunk = b"".join(PP._page_header(n, len(region), enc) + bytes(region) for enc, region, n in pages)
    rows = sum(n for _, _, n in pages)
    stage = PP.StagedDelta(len(chunk) + 64, 4, rows // 32 + 8)
    vals = torch.full((rows,), -7, dtype=torch.int32 if ptype in (1, 4) else torch.int64)
    r, v, need = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)()
    rc = lib.nvt_pq_decode_chunk_delta((C.c_uint8 * len(chunk)).from_buffer_copy(chunk), len(chunk), 0, ptype, 0, rows,
                                       None, 0, vals.data_ptr(), vals.numel() * vals.element_size(), 0,
                                       C.byref(stage.c), None, 0, C.byref(r), C.byref(v), need)
    return rc, lib.nvt_last_error().decode(), stage, vals


def mixed_chunk():
    """PLAIN, delta, PLAIN, delta pages in ONE int64 chunk (parquet-mr's fallback shape and more)."""
    x = np.cumsum(np.random.default_rng(9).integers(-3, 1 << 33, 700))
    cuts = [(0, 0, 200), (5, 200, 500), (0, 500, 600), (5, 600, 700)]
    pages = [(enc, DR.encode(x[a:b], 64) if enc else x[a:b].tobytes(), b - a) for enc, a, b in cuts]
    return x, _decode_chunk(pages, ptype=2)


def test_plain_pages_beside_delta_pages_keep_their_values_and_leave_holes():
    x, (rc, msg, stage, vals) = mixed_chunk()
    assert rc == 0, msg
    _, pos, count, _, _ = KPD.page_records(stage)
    assert pos.tolist() == [200, 600] and count.tolist() == [300, 100]
    want = np.full(700, -7)
    want[:200], want[500:600] = x[:200], x[500:600]
    np.testing.assert_array_equal(vals.numpy(), want)      # the holes are untouched
    at = stage.pages[: W * 2].numpy().reshape(-1, W)[:, 4]
    for p, (a, b) in enumerate([(200, 500), (600, 700)]):
        np.testing.assert_array_equal(DR.decode(stage.bytes.numpy()[int(at[p]): stage.nbytes], 64), x[a:b])


def test_corrupt_delta_pages_are_errors():
    x = np.random.default_rng(5).integers(-2**31, 2**31, 300).astype(np.int32)
    good = DR.encode(x, 32)
    head = len(DR._varint(128) + DR._varint(4) + DR._varint(300) + DR._zigzag(int(x[0])))
    rc, _, stage, _ = _decode_chunk([(5, good, 300)])
    assert rc == 0 and stage.npages == 1 and stage.nmbs == 10   # (299 deltas: 10 miniblocks of 32)
    min_delta = len(DR._zigzag(int(min(DR._signed(int(b) - int(a), 32) for a, b in zip(x[:127], x[1:128])))))
    wide = bytearray(good)
    assert wide[head + min_delta] == 32
    wide[head + min_delta] = 33                                # a width byte above the type's bits
    count = bytearray(good)
    count[3:5] = DR._varint(301)                               # total_count != what the levels say
    cut = good[: len(good) - 5]                                # the page ends inside its last miniblock
    for bad, what in ((wide, "bit width 33"), (count, "301 values"), (cut, "runs past")):
        rc, msg, stage, _ = _decode_chunk([(5, bad, 300)])
        assert rc == _lib.NVT_EINVAL and what in msg and stage.npages == 0, (rc, msg)
    rc, msg, _, _ = _decode_chunk([(5, good, 300)], ptype=4)   # a FLOAT chunk that claims encoding 5
    assert rc == _lib.NVT_EINVAL and "INT32 / INT64" in msg
