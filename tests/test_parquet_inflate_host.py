"""Snappy pages, host half: ``read_row_groups_staged(device_inflate=True)`` stages exactly the PLAIN
pages known to hold no nulls; their bodies inflate to the bytes the host route writes at the holes, and
everything outside the holes equals the host route's output."""
import numpy as np
import pyarrow as pa
import pytest

import inflate_reference as IR
from nvtabular_amd import _lib
from nvtabular_amd import parquet_plain as PP
from snappy_reference import read_varint


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_staged_bodies_inflate_to_what_the_host_route_decodes(tmp_path, version, nullable):
    path = str(tmp_path / "z.parquet")
    IR.write(path, version, nullable, with_nulls=("f64",))
    pf = PP.PlainParquetFile(path)
    assert pf.decodable and pf.num_row_groups == 2, pf.why_pyarrow
    eligible = IR.eligible_pages(path)
    # (a v2 page that does not shrink, like the float32 normals, is stored as it is and is not eligible)
    assert all(eligible[c] >= 4 for c in ("i32", "i64", "ts")), eligible
    counted = PP.READER_CHUNKS["inflate_pages"]
    staged = PP.read_row_groups_staged(pf, [0, 1], pin=False, device_inflate=True)
    host = PP.read_row_groups_staged(pf, [0, 1], pin=False)
    assert PP.READER_CHUNKS["inflate_pages"] - counted == sum(eligible.values())
    for name in IR.NUMBER_COLUMNS:
        sc, hc = staged[name], host[name]
        assert hc.inflate is None and sc.nvalid == hc.nvalid and (sc.valid is None) == (hc.valid is None), name
        assert (sc.inflate.npages if sc.inflate is not None else 0) == eligible[name], name
        if sc.valid is not None:
            assert bytes(sc.valid.numpy()) == bytes(hc.valid.numpy()), name
        want = hc.values[: hc.nvalid].numpy().view(np.uint8)
        got = sc.values[: sc.nvalid].numpy().view(np.uint8)
        hole = np.zeros(want.size, dtype=bool)
        for src_at, src_bytes, dst_at, dst_bytes, flags in (sc.inflate.records() if sc.inflate is not None else ()):
            body = bytes(sc.inflate.bytes[src_at: src_at + src_bytes].numpy())
            levels = version == "1.0" and pf.max_def[pf.names.index(name)] == 1
            assert src_at % 16 == 0 and flags == (_lib.INFLATE_V1_LEVELS if levels else 0), name
            raw = pa.decompress(body, decompressed_size=read_varint(body)[0], codec="snappy", asbytes=True)
            if flags:
                raw = raw[4 + int.from_bytes(raw[:4], "little"):]
            assert len(raw) == dst_bytes and raw == want[dst_at: dst_at + dst_bytes].tobytes(), name
            assert not hole[dst_at: dst_at + dst_bytes].any()
            hole[dst_at: dst_at + dst_bytes] = True
        np.testing.assert_array_equal(got[~hole], want[~hole], err_msg=name)
