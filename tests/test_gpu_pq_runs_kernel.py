"""nvt_pq_expand_runs against the numpy restatement (pq_runs_reference.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import pq_runs_reference as R
from nvtabular_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 256   # int32 words of -7 on both sides of `out`
WIDTHS = (1, 2, 3, 7, 8, 9, 16, 17, 24, 31, 32)


def run_kernel(runs, packed, entries, nvalues=None, closing=None):
    """-> (rc, ids, bad) of one call; `out` lies between guard words that must come back intact."""
    lib = _lib.load()
    runs = np.ascontiguousarray(runs, dtype=np.uint32).reshape(-1, 4)
    nvalues = int(runs[-1, 0]) if nvalues is None else nvalues
    closing = runs[-1].copy() if closing is None else np.asarray(closing, dtype=np.uint32)
    d_runs = torch.from_numpy(runs.view(np.int32).reshape(-1).copy()).cuda()
    d_packed = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.uint8)).cuda()
    buf = torch.full((nvalues + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.nvt_pq_expand_runs(d_runs.data_ptr(), len(runs) - 1, closing.ctypes.data, d_packed.data_ptr(),
                                d_packed.numel(), entries, nvalues, buf.data_ptr() + 4 * GUARD, bad.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == -7).all() and (host[GUARD + nvalues:] == -7).all()
    return rc, host[GUARD: GUARD + nvalues], int(bad.cpu().numpy()[0])


def check(runs, packed, entries):
    want, want_bad = R.expand(runs, packed, entries)
    rc, got, bad = run_kernel(runs, packed, entries)
    assert rc == 0, _lib.load().nvt_last_error()
    np.testing.assert_array_equal(got, want)
    assert bad == want_bad
    return got, bad


@pytest.mark.parametrize("width", WIDTHS)
def test_every_width(width):
    rng = np.random.default_rng(width)
    entries = min(1 << width, (1 << 31) - 1)
    tb = R.TableBuilder()
    for n in (5000, 3, 64):
        tb.packed_run(rng.integers(0, entries, n, dtype=np.uint64), width)
    got, bad = check(*tb.done(), entries)
    assert bad == 0 and got.max() < entries


@pytest.mark.parametrize("nvalues", [1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_random_mixes_of_the_three_kinds(nvalues):
    rng = np.random.default_rng(nvalues)
    for max_run in (3, 300):
        runs, packed = R.random_table(rng, nvalues, 70_000, WIDTHS, max_run=max_run)
        assert {int(k) & 0xFF for k in runs[:-1, 1]} <= {R.REPEAT, R.PACKED, R.SEQUENCE}
        got, bad = check(runs, packed, 70_000)
        assert bad == 0 and len(got) == nvalues


def test_a_tile_of_one_value_runs_and_a_run_across_the_tile_edge():
    tb = R.TableBuilder()
    for i in range(2048):                       # 2048 runs fill the first tile exactly
        tb.repeat(i % 97, 1) if i % 2 else tb.sequence(i, 1)
    tb.packed_run(np.arange(3000, dtype=np.uint64) % 500, 9)   # crosses the edge of the second tile
    tb.repeat(5, 10)
    got, bad = check(*tb.done(), 5000)
    assert bad == 0


def test_one_run_over_more_than_three_tiles():
    rng = np.random.default_rng(1)
    tb = R.TableBuilder()
    tb.repeat(3, 100)
    tb.packed_run(rng.integers(0, 1 << 17, 7000, dtype=np.uint64), 17)
    tb.sequence(10, 6500)
    check(*tb.done(), 1 << 17)


def test_a_clipped_packed_run():
    """Parquet pads the last group of 8: the bytes hold 16 values, the run owes 11 of them."""
    tb = R.TableBuilder()
    tb.packed_run(np.arange(16, dtype=np.uint64), 5, clip=11)
    tb.repeat(1, 4)
    got, bad = check(*tb.done(), 16)
    assert got.tolist() == list(range(11)) + [1] * 4 and bad == 0


def test_two_chunks_with_entry_bases():
    rng = np.random.default_rng(2)
    tb = R.TableBuilder()
    a, b = rng.integers(0, 1000, 3000, dtype=np.uint64), rng.integers(0, 128, 2500, dtype=np.uint64)
    tb.packed_run(a, 10, base=0)
    tb.packed_run(b, 7, base=1000)
    got, bad = check(*tb.done(), 1128)
    assert bad == 0
    np.testing.assert_array_equal(got, np.concatenate([a, b + 1000]).astype(np.int32))


def test_bad_ids_are_minus_one_and_counted():
    tb = R.TableBuilder()
    vals = np.array([0x80000000, 5, 0xFFFFFFFF, 0x7FFFFFFF, 6, 0x80000001, 7, 8], dtype=np.uint64)
    tb.packed_run(vals, 32)                     # width 32 with the top bit set
    tb.repeat(0xFFFFFFFF, 100)                  # the host decoder's mark for an index past its dictionary
    tb.sequence(95, 10)                         # runs out of the entries half way
    tb.packed_run(np.arange(2048 + 70, dtype=np.uint64) % 4, 2, base=98)
    runs, packed = tb.done()
    got, bad = check(runs, packed, 100)
    assert got[:8].tolist() == [-1, 5, -1, -1, 6, -1, 7, 8]
    assert (got[8:108] == -1).all() and got[108:118].tolist() == [95, 96, 97, 98, 99, -1, -1, -1, -1, -1]
    assert bad == 4 + 100 + 5 + int(((np.arange(2118) % 4) >= 2).sum())


def test_reads_stay_inside_the_packed_bytes():
    """A record that points past the staged bytes gives bad ids, not reads: the table is data."""
    tb = R.TableBuilder()
    tb.packed_run(np.arange(64, dtype=np.uint64), 8)
    runs, packed = tb.done()
    runs[0, 3] = 0x3FFFFFFF                      # word position far outside
    got, bad = check(runs, packed, 256)
    assert bad == 64 and (got == -1).all()


def test_no_values_and_refused_arguments():
    lib = _lib.load()
    tb = R.TableBuilder()
    tb.repeat(1, 10)
    runs, packed = tb.done()
    empty = np.array([[0, R.END, 0, 0]], dtype=np.uint32)
    rc, got, bad = run_kernel(empty, packed, 5)
    assert rc == 0 and len(got) == 0 and bad == 0
    # the closing record does not say nvalues
    rc, got, _ = run_kernel(runs, packed, 5, nvalues=9)
    assert rc == _lib.NVT_EINVAL and b"closing" in lib.nvt_last_error() and (got == -7).all()
    rc, got, _ = run_kernel(runs, packed, 5, closing=[10, R.REPEAT, 0, 0])
    assert rc == _lib.NVT_EINVAL and (got == -7).all()
    # null pointers
    closing = runs[-1].copy()
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_runs = torch.from_numpy(runs.view(np.int32).reshape(-1).copy()).cuda()
    d_packed = torch.from_numpy(packed).cuda()
    args = [d_runs.data_ptr(), 1, closing.ctypes.data, d_packed.data_ptr(), d_packed.numel(), 5, 10, out.data_ptr(),
            word.data_ptr(), None]
    for k in (0, 2, 3, 7, 8):
        bad_args = list(args)
        bad_args[k] = None
        assert lib.nvt_pq_expand_runs(*bad_args) == _lib.NVT_EINVAL and b"null" in lib.nvt_last_error()
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
