"""Ordering a vocabulary THROUGH THE SLOTS the counting pass recorded (nvt_vocab_col.src_slots: the
class scatter of csrc/nvt_vocab_order.hip stores every label into its table slot) against ordering it
through the patch pass (no slots: range_patch_many_kernel streams over the whole dumped table).

Both run on copies of the same dumped table, the same key-sorted list and histogram; the two tables
are compared byte for byte -- every slot, the empty ones and the kRpGuard words included -- together
with the ordered keys, the ordered counts and the label of the smallest int32, and the ordered list
is compared with numpy's "count descending, key ascending".  The counts of the source list are set by
the test (the dumped table holds positions, not counts), so a shape costs one count of n rows.

Then Categorify fit + transform on the range path against the oracle: one partition (dumped table,
slots) and two partitions (the merged list has no slots: flat table)."""
import contextlib
import zlib

import numpy as np
import pandas as pd
import pytest
import torch

import oracle as O
import order_reference as R

pytestmark = pytest.mark.gpu

LO = np.iinfo(np.int32).min
TILE, ORD_BATCH = 4096, 16          # kS2Tile, kOrdBatch
RESIDENT = 8192                     # NVT_ENCODE_RESIDENT_I32
REGION, GUARD = 16384 + 128, 64     # kRpRegion, kRpGuard


@pytest.fixture(scope="module")
def K():
    from nvtabular_amd import kernels

    return kernels


@pytest.fixture(scope="module", autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def rng_of(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sorted_keys(n, rng, lo):
    """n distinct keys spread over [0, 2^31), sorted; (lo) the smallest int32 in front."""
    m = n - bool(lo)
    k = (np.arange(1, m + 1, dtype=np.int64) * 2654435761 + 12345 + int(rng.integers(0, 1000))) % (2**31)
    return np.sort(np.append(k, LO) if lo else k).astype(np.int32)


def count_all(K, key_lists, rng):
    """Every list counted on the range path at 256 buckets, each key once: [(keys, counts, info)] with the
    dumped table and the slots."""
    jobs = []
    for keys in key_lists:
        job = K.DenseCountJob(dev(rng.permutation(keys)), None, None, hint=20_000, min_range_bits=8)
        job.path = K.PATH_RANGE
        jobs.append(job)
    out = []
    for keys, (dk, dc, nulls, info) in zip(key_lists, K.dense_count_many(jobs)):
        assert info["path"] == K.PATH_RANGE and info["range_bits"] == 8 and nulls == 0, info
        assert info["range_table"] is not None and info["range_slots"] is not None
        np.testing.assert_array_equal(dk.cpu().numpy(), keys)
        out.append((dk, dc, info))
    return out


@contextlib.contextmanager
def resident_gate(K, lifted):
    old = K.ENCODE_RESIDENT_I32
    if lifted:
        K.ENCODE_RESIDENT_I32 = 0      # (a table object for a vocabulary that would be encoded from LDS)
    try:
        yield
    finally:
        K.ENCODE_RESIDENT_I32 = old


class Job:
    """One vocabulary of a finalize call.  mode: slots | patch | flat."""

    def __init__(self, keys, counts, counted, mode, first=3):
        self.keys, self.counts, self.counted, self.mode, self.first = keys, counts, counted, mode, first

    def fill(self, K, d):
        dk, _, info = self.counted
        dc = dev(self.counts)
        hist = K.class_hist(dc)
        rtab = None
        if self.mode != "flat":
            rtab = (info["range_table"].clone(), info["range_aux"], info["range_bits"])
            if self.mode == "slots":
                rtab += (info["range_slots"],)
        ok, self.oc = torch.empty_like(dk), torch.empty_like(dc)
        lifted = self.keys.size <= RESIDENT
        with resident_gate(K, lifted):
            self.tab = tab = K.EncodeTable(ok, self.first, unique=True, defer_build=True, range_table=rtab,
                                           flat=self.mode == "flat")
        assert tab.kind == ("flat" if self.mode == "flat" else "dumped")
        if lifted:
            tab.head_image = None
        tab.fill_vocab_desc(d, self.oc, int(self.counts.max()), src=(dk, dc, hist, R.n_big_ref(self.counts), None))
        assert (d.src_slots is not None) == (self.mode == "slots"), self.mode

    def result(self):
        self.tab.wait_ready()
        torch.cuda.synchronize()
        return (self.tab._vk.cpu().numpy(), self.oc.cpu().numpy(), int(self.tab.sentinel_label.item()),
                self.tab.table)


def finalize(K, jobs):
    from nvtabular_amd import _lib

    descs = (_lib.VocabCol * len(jobs))()
    for d, j in zip(descs, jobs):
        j.fill(K, d)
    K.check(_lib.load().nvt_vocab_finalize_many(descs, len(jobs), K.stream_ptr()), "nvt_vocab_finalize_many")
    return [j.result() for j in jobs]


def check_order(job, res, what):
    vk, vc = R.vocab_order_ref(job.keys, job.counts)
    R.first_mismatch(res[0], vk, what + ": vocabulary order")
    R.first_mismatch(res[1], vc, what + ": ordered counts")
    assert res[2] == int(R.labels_ref(np.array([LO], np.int32), vk, job.first)[0]), what + ": label of the smallest int32"


def same_tables(a, b, what):
    """Byte for byte, on the device; the first differing slot is named."""
    assert a.numel() == b.numel() == (256 * REGION + GUARD) * 8
    if not torch.equal(a, b):
        wa, wb = a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64)
        at = int(np.flatnonzero(wa != wb)[0])
        raise AssertionError(f"{what}: slot {at} holds {int(wa[at]):#x} through the slots, {int(wb[at]):#x} "
                             f"through the patch pass ({int((wa != wb).sum())} slots differ)")


def both_ways(K, keys, counts, counted, what):
    a, b = Job(keys, counts, counted, "slots"), Job(keys, counts, counted, "patch")
    ra = finalize(K, [a])[0]
    rb = finalize(K, [b])[0]
    check_order(a, ra, what + " [slots]")
    check_order(b, rb, what + " [patch]")
    same_tables(ra[3], rb[3], what)
    return ra


def below_tail(n, rng):
    return np.minimum(rng.zipf(1.6, n), 250).astype(np.int64)


def shape(name, rng):
    """(keys, counts) of a named shape."""
    if name == "one entry":
        return sorted_keys(1, rng, False), np.array([3], np.int64)
    if name.startswith("tile"):
        n = TILE + {"tile-1": -1, "tile": 0, "tile+1": 1}[name]
        keys = sorted_keys(n, rng, lo=n % 2 == 1)
        counts = below_tail(n, rng)
        counts[1 + rng.permutation(n - 1)[:6]] = [255, 400, 255, 1000, 256, 400]
        return keys, counts
    n = 9001
    lo = name in ("sentinel in class 255", "sentinel below class 255")
    keys = sorted_keys(n, rng, lo)
    counts = below_tail(n, rng)
    at = 1 + rng.permutation(n - 1)
    if name != "class 255 empty":
        counts[at[:9]] = [255, 255, 400, 400, 400, 9000, 256, 70_000, 255]      # ties: the key order decides
    if lo:
        counts[0] = 400 if name == "sentinel in class 255" else 2
    return keys, counts


SHAPES = ["one entry", "tile-1", "tile", "tile+1", "class 255 empty", "class 255 with ties",
          "sentinel in class 255", "sentinel below class 255"]


@pytest.fixture(scope="module")
def counted_shapes(K):
    """All shapes counted by ONE dense_count_many call, shared by the cases below and never changed
    (every finalize call works on a clone of the table)."""
    lists = {}
    for name in SHAPES:
        lists[name] = shape(name, rng_of("shape", name))
    counted = count_all(K, [lists[n][0] for n in SHAPES], rng_of("rows"))
    return {n: (lists[n][0], lists[n][1], c) for n, c in zip(SHAPES, counted)}


@pytest.mark.parametrize("name", SHAPES)
def test_slots_equal_the_patch_pass(K, counted_shapes, name):
    keys, counts, counted = counted_shapes[name]
    n_big = R.n_big_ref(counts)
    assert (n_big == 0) == (name in ("one entry", "class 255 empty")), (name, n_big)
    if name.startswith("sentinel"):
        assert keys[0] == LO and (counts[0] >= 255) == (name == "sentinel in class 255")
    res = both_ways(K, keys, counts, counted, name)
    # the table is complete: every key of the vocabulary but the smallest int32, under its label
    words = res[3].cpu().numpy().view(np.uint64)
    words = words[(words & 0xFFFFFFFF) != 0x80000000]
    got = (words & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    o = np.argsort(got, kind="stable")
    in_table = keys[keys != LO]
    R.first_mismatch(got[o], in_table, name + ": keys in the table")
    R.first_mismatch((words >> 32).astype(np.int64)[o], R.labels_ref(in_table, res[0], 3), name + ": labels in the table")


def test_a_batch_with_slots_without_slots_and_a_flat_job(K, counted_shapes):
    """Three vocabularies in one batched call: a dumped table with slots, one without (the patch pass
    still runs, for that job alone), a flat table.  Each equals what it gives alone."""
    picks = ["class 255 with ties", "sentinel in class 255", "tile+1"]
    for modes in (["slots", "patch", "flat"], ["slots", "slots", "slots"], ["patch", "flat", "patch"]):
        jobs = [Job(*counted_shapes[p][:2], counted_shapes[p][2], m, first=3 + i)
                for i, (p, m) in enumerate(zip(picks, modes))]
        got = finalize(K, jobs)
        for j, r, p in zip(jobs, got, picks):
            what = f"{p} [{j.mode}] in a batch of {modes}"
            check_order(j, r, what)
            if j.mode != "flat":
                alone = Job(j.keys, j.counts, j.counted, "patch", first=j.first)
                same_tables(r[3], finalize(K, [alone])[0][3], what)


def test_more_jobs_than_one_batch_takes(K):
    """kOrdBatch + 1 dumped vocabularies, every third without slots: two batches."""
    rng = rng_of("seventeen")
    sizes = [300 + 577 * i for i in range(ORD_BATCH + 1)]
    lists = []
    for i, n in enumerate(sizes):
        keys = sorted_keys(n, rng, lo=i % 4 == 0)
        counts = below_tail(n, rng)
        counts[1 + rng.permutation(n - 1)[:i % 5]] = 255 + rng.integers(0, 50, i % 5)
        lists.append((keys, counts))
    counted = count_all(K, [k for k, _ in lists], rng)
    jobs = [Job(k, c, cn, "patch" if i % 3 == 2 else "slots", first=3 + i)
            for i, ((k, c), cn) in enumerate(zip(lists, counted))]
    got = finalize(K, jobs)
    alone = [Job(j.keys, j.counts, j.counted, "patch", first=j.first) for j in jobs]
    ref = finalize(K, alone)
    for j, r, rr in zip(jobs, got, ref):
        what = f"vocabulary of {j.keys.size} entries [{j.mode}] among {len(jobs)}"
        check_order(j, r, what)
        same_tables(r[3], rr[3], what)


# ---------------------------------------------------------------------------------------------
# the workflow
# ---------------------------------------------------------------------------------------------
def zipf_keys(rng, n, card, s=1.1):
    u = rng.random(n)
    x = np.floor(((card ** (1.0 - s) - 1.0) * u + 1.0) ** (1.0 / (1.0 - s))).clip(1, card).astype(np.int64)
    return ((x * 2654435761 + 12345) % (2**31)).astype(np.int32)


@pytest.mark.parametrize("nparts", [1, 2])
def test_workflow_on_the_range_path_vs_oracle(K, tmp_path, monkeypatch, nparts):
    """A small frame sent to the range path by its hint.  One partition: the dumped table is labelled
    through the slots; two partitions: the merged list carries none and gets a flat table.  Labels,
    unique.* files and embedding sizes equal the oracle's."""
    import nvtabular_amd as nvt
    from nvtabular_amd import ops

    rng = rng_of("workflow", nparts)
    n = 150_000
    parts = []
    for _ in range(nparts):
        v = zipf_keys(rng, n, 60_000)
        v[rng.integers(0, n, 3)] = LO                      # the smallest int32 is a key like any other
        parts.append(pd.DataFrame({"c": v}))
    seen = []
    fill = K.EncodeTable.fill_vocab_desc

    def spy(self, d, *args, **kw):
        fill(self, d, *args, **kw)
        seen.append((self.kind, d.src_slots is not None))

    monkeypatch.setattr(K.EncodeTable, "fill_vocab_desc", spy)
    cat = ops.Categorify(out_path=str(tmp_path / "g"))
    cat._cap_hints.update({"c#0": 120_000})                # beyond the LDS paths: the range path
    wf = nvt.Workflow(["c"] >> cat)
    wf.fit(nvt.Dataset(parts))
    got = wf.transform(nvt.Dataset(parts)).to_ddf().compute()
    assert cat._last_paths["c#0"] == K.PATH_RANGE
    assert seen == [("dumped", True)] if nparts == 1 else seen == [("flat", False)], seen
    oparts = parts
    paths = O.categorify_fit(oparts, ["c"], str(tmp_path / "c"), tie_break="stable")
    exp = O.categorify_transform(pd.concat(oparts, ignore_index=True), ["c"], paths)
    np.testing.assert_array_equal(got["c"].to_numpy(), exp["c"].to_numpy())
    a = pd.read_parquet(tmp_path / "g" / "categories" / "unique.c.parquet")
    b = pd.read_parquet(paths["c"])
    np.testing.assert_array_equal(a["c"].to_numpy().astype(np.int64), b["c"].to_numpy().astype(np.int64))
    np.testing.assert_array_equal(a["c_size"].to_numpy(), b["c_size"].to_numpy())
    card, dim = O.embedding_sizes(paths, ["c"], None)["c"]
    assert wf.output_schema["c"].properties["embedding_sizes"] == {"cardinality": card, "dimension": dim}
