"""nvt_pq_dict_fill_many on hand-built stages against its numpy restatement (tests/dict_in_reference.py):
every run shape and column length of a (value size, bit width, dictionary size) case is one column of ONE
call; guard words around the values and the positions of KEEP runs must come back untouched."""
import numpy as np
import pytest
import torch

import dict_in_reference as DI
from nvtabular_amd import _lib
from nvtabular_amd import kernels_parquet_dict_in as KDI

pytestmark = pytest.mark.gpu

T, LDS = _lib.PQ_DICT_TILE, _lib.PQ_DICT_LDS_BYTES
REPEAT, PACKED, KEEP, END = _lib.PQ_RUN_REPEAT, _lib.PQ_RUN_PACKED, _lib.PQ_RUN_KEEP, _lib.PQ_RUN_END
LENGTHS = [1, T - 1, T, T + 1, 3 * T + 5]
SHAPES = {"repeat": [(REPEAT, 700)], "packed": [(PACKED, 1 << 30)], "short": [(REPEAT, 0)],
          "offtile": [(PACKED, 1000), (REPEAT, 3333), (PACKED, 777)], "gap": [(PACKED, 1500), (KEEP, 901), (PACKED, 1 << 30)]}


def _stage(rng, size, width, total, n, shape, spoil=()):
    """One hand-built column: (recs, packed, dct) with ``total`` dictionary elements (the head included)
    and ``n`` values cut into the runs of ``shape`` (cycled; length 0: 1 .. 8 at random); ``spoil``:
    {value position: index} overrides inside packed runs."""
    a0, ndict = 16 // size, total - 16 // size
    dct = rng.integers(1, 1 << 62, total).astype(f"u{size}")
    dct[:a0] = np.frombuffer(np.array([ndict, 0], dtype=np.uint64).tobytes(), dtype=dct.dtype)
    top = min(ndict, 1 << width)
    recs, packed, at, k = [], bytearray(), 0, 0
    while at < n:
        kind, length = SHAPES[shape][k % len(SHAPES[shape])]
        length = min(length or int(rng.integers(1, 9)), n - at)
        if kind == PACKED:
            idx = rng.integers(0, top, length).astype(np.uint64)
            for q, v in spoil:
                if at <= q < at + length:
                    idx[q - at] = v
            bits = ((idx[:, None] >> np.arange(width, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)
            recs.append((at, PACKED | width << 8, a0, len(packed) // 4))
            packed += np.packbits(bits, bitorder="little").tobytes()
            packed += bytes(-len(packed) % 4)
        else:
            recs.append((at, kind, a0 + int(rng.integers(0, ndict)) if kind == REPEAT else 0, 0))
        at, k = at + length, k + 1
    recs.append((n, END, 0, 0))
    packed += bytes(8 + (-(len(packed) + 8) % 16))
    return np.array(recs, dtype=np.uint32), np.frombuffer(bytes(packed), dtype=np.uint8), dct


def _run(stages):
    """Fills all ``stages`` (recs, packed, dct, n) in one call; -> bad, and checks values + guards."""
    dev, cols, checks = torch.device("cuda:0"), [], []
    for recs, packed, dct, n in stages:
        g = 16 // dct.itemsize   # 16 bytes of guard words on either side
        want = np.full(n + 2 * g, 0xA5A5A5A5A5A5A5A5 >> (64 - 8 * dct.itemsize), dtype=dct.dtype)
        buf = torch.from_numpy(want.copy().view(f"i{dct.itemsize}")).to(dev)
        checks.append((buf, want, DI.fill(recs, packed, dct, want[g: g + n])))
        cols.append((torch.from_numpy(recs.view(np.int32).reshape(-1)).to(dev), len(recs) - 1,
                     torch.from_numpy(packed.copy()).to(dev), torch.from_numpy(dct.view(np.uint8).copy()).to(dev),
                     len(dct), buf[g: g + n]))
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    KDI.fill_many(cols, bad)
    for i, (buf, want, _) in enumerate(checks):
        np.testing.assert_array_equal(buf.cpu().numpy().view(want.dtype), want, err_msg=f"column {i}")
    assert int(bad.cpu()[0]) == sum(b for _, _, b in checks)
    return int(bad.cpu()[0])


@pytest.mark.parametrize("ndict", ["one", "under", "fits", "over"])
@pytest.mark.parametrize("width", [1, 3, 8, 17, 32])
@pytest.mark.parametrize("size", [4, 8])
def test_fill_equals_numpy(size, width, ndict):
    rng = np.random.default_rng(width * 16 + size)
    total = {"one": 16 // size + 1, "under": LDS // size - 1, "fits": LDS // size, "over": LDS // size + 1}[ndict]
    stages = [_stage(rng, size, width, total, n, shape) + (n,) for n in LENGTHS for shape in SHAPES]
    assert _run(stages) == 0


def test_columns_of_different_value_sizes_in_one_call():
    rng = np.random.default_rng(1)
    stages = [_stage(rng, size, width, total, n, shape) + (n,) for size, width, total, n, shape in
              ((4, 5, 40, 2 * T + 3, "offtile"), (8, 17, LDS // 8 + 9, 3 * T + 5, "gap"), (4, 32, 900, T + 1, "short"))]
    assert _run(stages) == 0


def test_indices_outside_the_dictionary_write_zero_and_are_counted():
    rng = np.random.default_rng(2)
    n = 2 * T + 9
    recs, packed, dct = _stage(rng, 8, 8, 100 + 2, n, "gap", spoil=((7, 200), (T + 4000, 100)))
    assert _run([(recs, packed, dct, n)]) == 2
