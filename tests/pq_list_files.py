"""The files of the parquet list reader's tests (tests/test_parquet_list_in_host.py,
tests/test_gpu_parquet_list_in.py): one session frame written four ways."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from nvtabular_amd import parquet_plain as PP


def session_table(seed=0):
    """1001 rows: 200 of 0 .. 3 leaves, 300 empty, 300 of one leaf, one of 500, 200 of 0 .. 3; every 97th
    row None, 20 % of the leaves null; int64 leaves, an int32 flat column and a float32 list beside."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(0, 4, 200), np.zeros(300, dtype=np.int64), np.ones(300, dtype=np.int64),
                           [500], rng.integers(0, 4, 200)]).astype(np.int64)
    assert len(lens) == 1001

    def lists(values_of, null_every):
        out = []
        for r, L in enumerate(lens):
            if r % null_every == 0:
                out.append(None)
                continue
            vals = values_of(int(L))
            out.append([None if rng.random() < 0.2 else v for v in vals])
        return out

    l = pa.array(lists(lambda L: [int(v) for v in rng.integers(0, 50, L)], 97), type=pa.list_(pa.int64()))
    f = pa.array(lists(lambda L: [float(np.float32(v)) for v in rng.normal(size=L)], 89), type=pa.list_(pa.float32()))
    x = pa.array(rng.integers(-9, 9, len(lens)).astype("int32"), mask=rng.random(len(lens)) < 0.1)
    return pa.table({"x": x, "l": l, "f": f})


WRITES = {
    "v1_plain": dict(use_dictionary=False, compression=None, data_page_size=1024, row_group_size=600),
    "default": dict(row_group_size=600),
    "v2": dict(data_page_version="2.0", data_page_size=1024, row_group_size=600),
}


def write_session_file(tmp_path, how):
    path = str(tmp_path / f"{how}.parquet")
    pq.write_table(session_table(), path, **WRITES[how])
    return path


def write_session_file_plain_writer(path, page_slots=200):
    """The session frame through this package's PlainParquetWriter, two row groups (the levels from
    the numpy restatement of the device packer: no GPU); the writer has no null lists, a None row is
    written as an empty one."""
    import pq_list_reference as W

    t = session_table()
    w = PP.PlainParquetWriter(path, ["x", "l", "f"], [np.int32, np.int64, np.float32], lists=[False, True, True])
    x = t["x"].combine_chunks()
    for r0, r1 in ((0, 600), (600, 1001)):
        cols = [(x.slice(r0, r1 - r0).drop_null().to_numpy(),
                 np.packbits(np.asarray(x.slice(r0, r1 - r0).is_valid()), bitorder="little"))]
        for name in ("l", "f"):
            col = t[name].combine_chunks()
            off = np.asarray(col.offsets).astype(np.int64)
            flat = col.flatten()
            valid = np.asarray(flat.is_valid())
            pages = W.list_pages(off, valid, r0, r1, page_slots)
            levels = PP.ListLevels([p["slots"] for p in pages], [p["nonnull"] for p in pages],
                                   np.frombuffer(b"".join(p["rep"] for p in pages), dtype=np.uint8),
                                   np.cumsum([0] + [len(p["rep"]) for p in pages])[:-1],
                                   np.frombuffer(b"".join(p["dfn"] for p in pages), dtype=np.uint8),
                                   np.cumsum([0] + [len(p["dfn"]) for p in pages])[:-1])
            lo, hi = int(off[r0]), int(off[r1])
            vals = flat.fill_null(0).to_numpy(zero_copy_only=False)[lo:hi][valid[lo:hi]]
            cols.append((np.ascontiguousarray(vals), levels))
        w.write_row_group(cols, r1 - r0)
    w.close()
    return path
