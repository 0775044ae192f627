"""numpy restatement of nvt_pq_dict_fill_many (include/nvt_hip.h, "parquet in: dictionary-encoded data
pages of flat 4- and 8-byte number columns") and the pyarrow files the dictionary-page tests read."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from nvtabular_amd import _lib

ROWS = 9000   # two row groups of 4500: more than one tile of 4096 values per chunk
KINDS = {"i32": pa.int32(), "i64": pa.int64(), "f32": pa.float32(), "f64": pa.float64(), "ts": pa.timestamp("us"),
         "i8": pa.int8(), "wide": pa.int64()}


def fill(recs, packed, dct, values):
    """``recs``: uint32 [nruns + 1, 4]; ``packed``: uint8; ``dct``: the staged dictionaries, heads
    included, as unsigned words of the value size; ``values``: the same words, written in place.
    -> the number of packed indices outside their chunk's entries (those positions become 0)."""
    bits = np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")
    size, bad = dct.itemsize, 0
    for (start, kw, a, b), end in zip(recs[:-1].tolist(), recs[1:, 0].tolist()):
        kind, width, n = kw & 0xFF, kw >> 8, end - start
        if kind == _lib.PQ_RUN_REPEAT:
            values[start:end] = dct[a]
        elif kind == _lib.PQ_RUN_PACKED:
            lim = int.from_bytes(dct.view(np.uint8)[a * size - 16: a * size - 8].tobytes(), "little")
            seg = bits[32 * b: 32 * b + n * width].reshape(n, width).astype(np.uint64)
            idx = (seg << np.arange(width, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            ok = idx < min(lim, len(dct) - a)
            values[start:end] = np.where(ok, dct[a + np.where(ok, idx, 0).astype(np.int64)], 0)
            bad += int((~ok).sum())
        else:
            assert kind == _lib.PQ_RUN_KEEP   # in place already
    return bad


def staged_words(sc):
    """The packed values of a StagedColumn read with device_dict, holes filled by ``fill``; -> (words, bad)."""
    words = sc.values[: sc.nvalid].numpy().copy().view(f"u{sc.values.element_size()}")
    st = sc.dict_stage
    if st is None:
        return words, 0
    recs = st.runs[: 4 * (st.nruns + 1)].numpy().view(np.uint32).reshape(-1, 4)
    hole = np.ones(len(words), dtype=bool)
    for (a, kw), b in zip(recs[:-1, :2].tolist(), recs[1:, 0].tolist()):
        hole[a:b] = (kw & 0xFF) != _lib.PQ_RUN_KEEP
    words[hole] = 0x5A   # (every value of a dictionary page must come out of the stage)
    dct = st.dict[: st.ndict_bytes].numpy().view(words.dtype)
    return words, fill(recs, st.packed[: st.npacked + 8].numpy(), dct, words)


def table(nullable):
    rng = np.random.default_rng(7)
    runs = np.repeat(rng.integers(0, 50, ROWS // 30 + 1), 30)[:ROWS]    # long RLE runs between packed ones
    f32 = rng.integers(0, 90, ROWS).astype(np.float32)
    f32[::17], f32[5::29] = np.float32("nan"), np.float32(-0.0)
    cols = {"i32": np.where(rng.random(ROWS) < 0.5, runs, rng.integers(-2**31, 2**31, 60)[runs]).astype(np.int32),
            "i64": rng.integers(-2**62, 2**62, 300)[rng.integers(0, 300, ROWS)],
            "f32": f32, "f64": rng.random(40)[rng.integers(0, 40, ROWS)],
            "ts": np.int64(1_700_000_000_000_000) + rng.integers(0, 2, ROWS),                   # bit width 1
            "i8": rng.integers(-128, 128, ROWS).astype(np.int8),
            "wide": np.concatenate([rng.integers(0, 40, 1500), rng.integers(0, 1 << 40, ROWS - 1500)])}   # overflows its dictionary
    arrays = [pa.array(v, type=KINDS[k], mask=(rng.random(ROWS) < 0.3) if nullable else None) for k, v in cols.items()]
    return pa.Table.from_arrays(arrays, schema=pa.schema([pa.field(k, t, nullable=nullable) for k, t in KINDS.items()]))


def write(path, nullable, compression, version):
    pq.write_table(table(nullable), path, use_dictionary=True, compression=compression, data_page_version=version,
                   data_page_size=1024, dictionary_pagesize_limit=4096, row_group_size=ROWS // 2)
    return pq.read_table(path)
