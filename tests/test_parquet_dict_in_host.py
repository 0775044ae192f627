"""Dictionary pages of number columns, host half: what ``read_row_groups_staged(device_dict=True)`` stages,
resolved with the numpy restatement of the device fill, equals pyarrow's columns bit for bit; the default
still resolves on the host; truncated chunks are errors and nothing is written outside the caller's arrays."""
import ctypes as C

import numpy as np
import pyarrow.parquet as pq
import pytest

import dict_in_reference as DI
from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP


def _want(col):
    """(valid mask, the non-null values as unsigned words of the physical size) of a pyarrow column."""
    col = col.combine_chunks()
    vals = col.drop_null().to_numpy(zero_copy_only=False)
    if vals.dtype.kind == "M":
        vals = vals.view(np.int64)
    if vals.dtype.itemsize < 4:
        vals = vals.astype(np.int32)   # (the file holds int8 / int16 as INT32)
    return np.asarray(col.is_valid()), vals.view(f"u{vals.dtype.itemsize}")


@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("nullable", [False, True])
def test_staged_dictionary_pages_resolve_to_pyarrows_columns(tmp_path, nullable, version, compression):
    path = str(tmp_path / "d.parquet")
    exp = DI.write(path, nullable, compression, version)
    pf = PP.PlainParquetFile(path)
    assert pf.decodable and pf.num_row_groups == 2, pf.why_pyarrow
    staged = PP.read_row_groups_staged(pf, [0, 1], pin=False, device_dict=True)
    host = PP.read_row_groups_staged(pf, [0, 1], pin=False)
    for name in DI.KINDS:
        sc, mask_vals = staged[name], _want(exp.column(name))
        mask, want = mask_vals
        assert sc.dict_stage is not None and host[name].dict_stage is None and sc.nvalid == len(want), name
        if nullable:
            np.testing.assert_array_equal(np.unpackbits(sc.valid.numpy(), bitorder="little")[:DI.ROWS].astype(bool), mask)
        got, bad = DI.staged_words(sc)
        assert bad == 0
        np.testing.assert_array_equal(got, want, err_msg=name)
        np.testing.assert_array_equal(host[name].values[: len(want)].numpy().view(want.dtype), want, err_msg=name)
    # several pages per chunk; the column that outgrows its dictionary has host-decoded PLAIN pages too
    kinds = staged["wide"].dict_stage.runs[1: 4 * staged["wide"].dict_stage.nruns: 4].numpy() & 0xFF
    assert {_lib.PQ_RUN_KEEP, _lib.PQ_RUN_PACKED} <= set(kinds.tolist())
    assert _lib.PQ_RUN_REPEAT in (staged["i32"].dict_stage.runs[1: 4 * staged["i32"].dict_stage.nruns: 4].numpy() & 0xFF)


@pytest.mark.parametrize("where", ["dictionary", "middle", "last byte"])
def test_truncated_chunks_are_errors_and_nothing_outside_the_arrays_is_touched(tmp_path, where):
    path = str(tmp_path / "t.parquet")
    DI.write(path, True, "snappy", "1.0")
    pf = PP.PlainParquetFile(path)
    cc, n = pf.row_groups[0]["columns"][pf.names.index("i64")], pf.row_groups[0]["num_rows"]
    raw = open(path, "rb").read()[cc["offset"]: cc["offset"] + cc["size"]]
    cut = {"dictionary": 40, "middle": len(raw) // 2, "last byte": len(raw) - 1}[where]
    guard, sbytes = 4096, 2 * max(cc["raw_size"], cc["size"]) + 64
    vals, bm, scr = (np.full(k + 2 * guard, 0xA5, dtype=np.uint8) for k in (n * 8, n // 8 + 16, sbytes))
    stage = PP.StagedDict(1 << 16, n, 1 << 16, False, "t")
    r, v, need = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)()
    buf = (C.c_uint8 * cut).from_buffer_copy(raw[:cut])
    rc = _lib.load().nvt_pq_decode_chunk_dict(buf, cut, cc["codec"], 8, 1, n, bm.ctypes.data + guard, 0,
                                              vals.ctypes.data + guard, n * 8, 0, C.byref(stage.c),
                                              scr.ctypes.data + guard, sbytes, C.byref(r), C.byref(v), need)
    with pytest.raises(_lib.NvtHipError):
        _lib.check(rc, "nvt_pq_decode_chunk_dict")
    assert rc == _lib.NVT_EINVAL and stage.nruns == 0 and stage.ndict_bytes == 0 and stage.npacked == 0
    for a in (vals, bm, scr):
        assert (a[:guard] == 0xA5).all() and (a[-guard:] == 0xA5).all()
