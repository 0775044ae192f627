"""PlainParquetWriter fed ``SnappyPages`` on the host (no GPU): the element bytes come from the
literal-only encoder of tests/snappy_reference.py and from pyarrow's codec (varint stripped).  pyarrow
reads the files back equal, the chunks say SNAPPY, their total_uncompressed_size is the size of the
same chunk written by the default path, and SNAPPY and UNCOMPRESSED chunks mix in one file.  The last
test takes ``Dataset.to_parquet(device_compression=...)`` on a frame on the host: argument errors,
and the codec handed to pyarrow."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import pq_dict_reference as D
import pq_list_reference as L
import pq_str_out_reference as S
import snappy_reference as R
from nvtabular_amd import parquet_plain as PP

PAGE = 100


def _elements(data, how):
    data = bytes(data)
    if not data:
        return b""
    if how == "literal":
        return R.encode_literal(data, piece=70)
    raw = pa.Codec("snappy").compress(data).to_pybytes()
    n, at = R.read_varint(raw)
    assert n == len(data)
    return raw[at:]


def _snap(dtype, region, cuts, how, **kw):
    """SnappyPages of a values region cut at the byte positions ``cuts``."""
    region = bytes(region)
    streams = [_elements(region[a:b], how) for a, b in zip(cuts[:-1], cuts[1:])]
    dense = np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8)[:-1]
    return PP.SnappyPages(dtype, dense, [len(s) for s in streams], np.diff(cuts), **kw)


def _levels(offsets, leaf_valid, n):
    pages = L.list_pages(offsets, leaf_valid, 0, n, PAGE)
    rep, dfn, rep_at, def_at = b"", b"", [], []
    for p in pages:
        rep_at.append(len(rep))
        def_at.append(len(dfn))
        rep += p["rep"]
        dfn += p["dfn"]
    return PP.ListLevels([p["slots"] for p in pages], [p["nonnull"] for p in pages], np.frombuffer(rep, dtype=np.uint8),
                         rep_at, np.frombuffer(dfn, dtype=np.uint8), def_at)


def _frame(n=250, seed=0):
    """The five column kinds as (plain columns, snappy-column makers, expected python values)."""
    rng = np.random.default_rng(seed)
    a = np.minimum(rng.zipf(1.3, n), 5000).astype(np.int64)                      # flat, no nulls
    b = rng.integers(0, 5, n).astype(np.float64)                                 # flat, nulls
    bv = rng.random(n) < 0.7
    lens = rng.integers(0, 4, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    leaves = rng.integers(0, 9, int(offsets[-1])).astype(np.int64)               # list, leaf nulls
    lv = rng.random(len(leaves)) < 0.8
    words = [None if rng.random() < 0.2 else "w%d" % rng.integers(0, 12) * int(rng.integers(1, 4)) for _ in range(n)]
    d = rng.integers(0, 7, n).astype(np.int64) * 1000                            # a dictionary chunk
    dv = rng.random(n) < 0.9
    return dict(a=a, b=b, bv=bv, offsets=offsets, leaves=leaves, lv=lv, words=words, d=d, dv=dv, n=n)


def _columns(f, how, snappy):
    """The row group's columns; ``snappy``: the set of column names handed over as SnappyPages."""
    n = f["n"]
    cols = {}
    cuts = [8 * x for x in D.flat_page_start(None, n, PAGE)]
    cols["a"] = (_snap(np.int64, f["a"].tobytes(), cuts, how) if "a" in snappy else f["a"], None)
    bvals, bbits = f["b"][f["bv"]], np.packbits(f["bv"], bitorder="little")
    cuts = [8 * x for x in D.flat_page_start(f["bv"], n, PAGE)]
    cols["b"] = (_snap(np.float64, bvals.tobytes(), cuts, how) if "b" in snappy else bvals, bbits)
    lev = _levels(f["offsets"], f["lv"], n)
    lvals = f["leaves"][f["lv"]]
    cuts = [8 * int(x) for x in np.concatenate([[0], np.cumsum(lev.nonnull)])]
    cols["l"] = (_snap(np.int64, lvals.tobytes(), cuts, how) if "l" in snappy else lvals, lev)
    body, page_at, nv, bitmap = S.byte_array_pages(f["words"], 96)
    cols["s"] = (_snap(PP.STRING_DTYPE, body.tobytes(), [int(x) for x in page_at], how, page_rows=96) if "s" in snappy
                 else PP.ByteArrayPages(body, page_at, nv, 96), bitmap)
    dvals, dbits = f["d"][f["dv"]], np.packbits(f["dv"], bitorder="little")
    dic, W, dnv, packed = D.encode(dvals, D.flat_page_start(f["dv"], n, PAGE))
    packed = np.frombuffer(packed + b"\0", dtype=np.uint8)[:-1]
    if "d" in snappy:
        cols["d"] = (_snap(np.int64, dic.tobytes(), [0, 8 * len(dic)], how, indices=(W, packed, dnv, len(dic))), dbits)
    else:
        cols["d"] = (PP.DictPages(dic, packed, W, dnv), dbits)
    return cols


def _write(path, frames, how, snappy):
    w = PP.PlainParquetWriter(str(path), list("ablsd"), [np.int64, np.float64, np.int64, PP.STRING_DTYPE, np.int64],
                              lists=[False, False, True, False, False])
    for f, which in zip(frames, snappy):
        cols = _columns(f, how, which)
        w.write_row_group([cols[k] for k in "ablsd"], f["n"])
    w.close()


def _expected(frames):
    out = {k: [] for k in "ablsd"}
    for f in frames:
        out["a"] += f["a"].tolist()
        out["b"] += [x if ok else None for x, ok in zip(f["b"].tolist(), f["bv"])]
        lv = iter(f["lv"].tolist())
        out["l"] += [[x if next(lv) else None for x in f["leaves"][s:e].tolist()]
                     for s, e in zip(f["offsets"][:-1], f["offsets"][1:])]
        out["s"] += f["words"]
        out["d"] += [x if ok else None for x, ok in zip(f["d"].tolist(), f["dv"])]
    return out


@pytest.fixture()
def small_pages(monkeypatch):
    monkeypatch.setattr(PP, "PAGE_VALUES", PAGE)


@pytest.mark.parametrize("how", ["literal", "pyarrow"])
def test_every_column_kind_reads_back_and_says_snappy(tmp_path, small_pages, how):
    frames = [_frame(250, 1), _frame(99, 2)]
    _write(tmp_path / "s.parquet", frames, how, [set("ablsd")] * 2)
    _write(tmp_path / "p.parquet", frames, how, [set()] * 2)
    got, plain = pq.read_table(tmp_path / "s.parquet"), pq.read_table(tmp_path / "p.parquet")
    assert got.equals(plain) and got.schema.equals(plain.schema)
    assert got.to_pydict() == _expected(frames)
    ms, mp = pq.read_metadata(tmp_path / "s.parquet"), pq.read_metadata(tmp_path / "p.parquet")
    assert ms.created_by == mp.created_by
    for g in range(2):
        assert ms.row_group(g).total_byte_size == mp.row_group(g).total_byte_size
        for j in range(5):
            cs, cp = ms.row_group(g).column(j), mp.row_group(g).column(j)
            assert cs.compression == "SNAPPY" and cp.compression == "UNCOMPRESSED"
            assert cs.total_uncompressed_size == cp.total_compressed_size == cp.total_uncompressed_size
            assert cs.encodings == cp.encodings and cs.num_values == cp.num_values
            assert (cs.dictionary_page_offset is None) == (cp.dictionary_page_offset is None)
            if how == "pyarrow" and j in (0, 2, 3):   # (label, leaf and string pages shrink)
                assert cs.total_compressed_size < cp.total_compressed_size
    f = PP.PlainParquetFile(str(tmp_path / "s.parquet"))
    assert f.decodable and all(c["codec"] == 1 for rg in f.row_groups for c in rg["columns"])


def test_snappy_and_uncompressed_chunks_mix_in_one_file(tmp_path, small_pages):
    frames = [_frame(250, 3), _frame(250, 4), _frame(7, 5)]
    which = [set("al"), set("bsd"), set("abd")]
    _write(tmp_path / "m.parquet", frames, "pyarrow", which)
    got = pq.read_table(tmp_path / "m.parquet")
    assert got.to_pydict() == _expected(frames)
    md = pq.read_metadata(tmp_path / "m.parquet")
    for g, names in enumerate(which):
        for j, k in enumerate("ablsd"):
            assert md.row_group(g).column(j).compression == ("SNAPPY" if k in names else "UNCOMPRESSED")


def test_size_arithmetic_is_the_layout(tmp_path, small_pages):
    """``snappy_chunk_bytes`` gives the chunk sizes the writer lays out, for both forms."""
    f = _frame(250, 6)
    _write(tmp_path / "s.parquet", [f], "pyarrow", [set("ablsd")])
    md = pq.read_metadata(tmp_path / "s.parquet").row_group(0)
    cols = _columns(f, "pyarrow", set("ablsd"))
    sp = cols["a"][0]
    rows = [100, 100, 50]
    pages = [(r, PP.flat_level_bytes(r, False), u, c, 0) for r, u, c in zip(rows, sp.raw, sp.sizes)]
    assert PP.snappy_chunk_bytes(pages) == (md.column(0).total_compressed_size, md.column(0).total_uncompressed_size)
    sp, lev = cols["l"]
    pages = [(s, PP.list_level_bytes(s), u, c, 0) for s, u, c in zip(lev.slots, sp.raw, sp.sizes)]
    assert PP.snappy_chunk_bytes(pages) == (md.column(2).total_compressed_size, md.column(2).total_uncompressed_size)
    sp = cols["d"][0]
    idx = [PP.dict_index_bytes([k], sp.W) for k in sp.nv]
    pages = [(r, PP.flat_level_bytes(r, True) + i, 0, 0, 8) for r, i in zip(rows, idx)]
    assert PP.snappy_chunk_bytes(pages, (sp.entries, sp.raw[0], sp.sizes[0])) == \
        (md.column(4).total_compressed_size, md.column(4).total_uncompressed_size)


def test_bad_snappy_pages_raise_before_anything_is_written(tmp_path, small_pages):
    f = _frame(250, 7)
    with pytest.raises(ValueError):
        PP.SnappyPages(np.int64, np.zeros(3, dtype=np.uint8), [4], [8])          # fewer dense bytes than the pages take
    with pytest.raises(ValueError):
        PP.SnappyPages(np.int64, np.zeros(8, dtype=np.uint8), [4, 4], [8])       # sizes and regions differ in number
    with pytest.raises(ValueError):
        PP.SnappyPages(np.int64, np.zeros(8, dtype=np.uint8), [0], [8])          # a region without a stream
    w = PP.PlainParquetWriter(str(tmp_path / "x.parquet"), ["a"], [np.int64])
    bad = _snap(np.int64, f["a"].tobytes(), [0, 800, 1600, 2000], "literal")
    with pytest.raises(ValueError):
        w.write_row_group([(bad, None)], 251)                                     # the regions do not match the rows
    with pytest.raises(TypeError):
        w.write_row_group([(_snap(np.int32, f["a"].tobytes(), [0, 800, 1600, 2000], "literal"), None)], 250)
    w.write_row_group([(bad, None)], 250)
    w.close()
    assert pq.read_table(tmp_path / "x.parquet").column("a").to_pylist() == f["a"].tolist()


def test_to_parquet_keyword_on_a_host_frame(tmp_path):
    """Argument errors come before anything is created; a frame on the host hands the codec to pyarrow;
    without the keyword the same frame is written as before."""
    import torch

    import nvtabular_amd as nvt
    from nvtabular_amd.device import DeviceColumn, DeviceFrame

    frame = DeviceFrame({"id": DeviceColumn(torch.arange(200, dtype=torch.int64)),
                         "x": DeviceColumn(torch.arange(200, dtype=torch.float64) / 4)})
    for name, kw in (("both", dict(compression="snappy", device_compression="snappy")),
                     ("zstd", dict(device_compression="zstd")), ("true", dict(device_compression=True))):
        with pytest.raises(ValueError, match="device_compression"):
            nvt.Dataset(frame).to_parquet(str(tmp_path / name), **kw)
        assert not (tmp_path / name).exists()
    nvt.Dataset(frame).to_parquet(str(tmp_path / "s"), device_compression="SNAPPY")
    md = pq.read_metadata(tmp_path / "s" / "part_0.parquet")
    assert md.created_by != "nvtabular_amd plain writer"
    assert all(md.row_group(0).column(j).compression == "SNAPPY" for j in range(2))
    nvt.Dataset(frame).to_parquet(str(tmp_path / "p"))
    md = pq.read_metadata(tmp_path / "p" / "part_0.parquet")
    assert md.created_by == "nvtabular_amd plain writer"
    assert all(md.row_group(0).column(j).compression == "UNCOMPRESSED" for j in range(2))
    assert pq.read_table(tmp_path / "s" / "part_0.parquet").equals(pq.read_table(tmp_path / "p" / "part_0.parquet"))
