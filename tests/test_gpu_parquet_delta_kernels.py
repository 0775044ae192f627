"""nvt_pq_delta_decode against tests/delta_reference.py, bit for bit: pages from the reference's encoder,
staged by the host walk (``StagedDelta.add_page``), decoded into holes whose surroundings must survive."""
import numpy as np
import pytest
import torch

import delta_reference as DR
from nvtabular_amd import kernels_parquet_delta as KPD
from nvtabular_amd import parquet_plain as PP

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 32, 33, 128, 129, 2048, 2049, 2048 * 3 + 5]   # no delta; miniblock, block, tile edges; carry
SENTINEL, dev = -0x5A5A5A5B, torch.device("cuda")


def _data(kind, bits, n):
    rng = np.random.default_rng(n * 7 + bits)
    if kind == "constant":        # all widths 0
        return np.full(n, -12345, dtype=f"int{bits}")
    if kind == "random":          # full-width deltas, wrap-around
        return rng.integers(-2**(bits - 1), 2**(bits - 1), n, dtype=f"int{bits}")
    steps = rng.integers(-5, 1000, n)   # increasing, with a negative min_delta
    return (np.cumsum(steps) - 2**20).astype(f"int{bits}")


def _decode(pages, bits, total, device):
    """pages: [(values, position of the hole)] of ONE column of ``total`` packed values."""
    stage = PP.StagedDelta(64, 1, 1)   # (far too small: grown page by page)
    for (values, pos), (block, minis) in pages:
        stage.add_page(DR.encode(values, bits, block, minis), bits // 8, len(values), pos)
    return stage, torch.full((total,), SENTINEL, dtype=getattr(torch, f"int{bits}"), device=device)


@pytest.mark.parametrize("shape", [(128, 4), (256, 4)], ids=["mb32", "mb64"])
@pytest.mark.parametrize("kind", ["constant", "random", "increasing"])
@pytest.mark.parametrize("bits", [32, 64])
def test_delta_decode_equals_the_reference(bits, kind, shape):
    items, want = [], []
    for n in COUNTS:   # every count is a column of its own: ONE call decodes them all
        x = _data(kind, bits, n)
        np.testing.assert_array_equal(DR.decode(DR.encode(x, bits, *shape), bits), x)   # the expected values
        stage, out = _decode([((x, 3), shape)], bits, n + 8, dev)
        items.append((stage, out))
        want.append(np.concatenate([np.full(3, SENTINEL, x.dtype), x, np.full(5, SENTINEL, x.dtype)]))
    KPD.fill_holes(items)
    for n, (_, out), exp in zip(COUNTS, items, want):
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg=f"count {n}")


def test_two_pages_of_one_column_in_holes_that_are_not_adjacent():
    a, b = _data("increasing", 64, 2049), _data("random", 64, 300)
    stage, out = _decode([((a, 10), (128, 4)), ((b, 10 + 2049 + 100), (256, 4))], 64, 2600, dev)
    narrow = _data("random", 32, 2048 * 2 + 1)   # a 32-bit column in the same call
    stage32, out32 = _decode([((narrow, 0), (256, 4))], 32, len(narrow) + 4, dev)
    KPD.fill_holes([(stage, out), (stage32, out32)])
    exp = np.full(2600, SENTINEL, np.int64)
    exp[10: 10 + 2049] = a
    exp[2159: 2159 + 300] = b
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    np.testing.assert_array_equal(out32.cpu().numpy(), np.concatenate([narrow, np.full(4, SENTINEL, np.int32)]))
