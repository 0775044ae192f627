"""Host-side logic that needs neither the GPU nor the shared library."""
import numpy as np


def test_estimate_distinct_model():
    from nvtabular_amd.kernels import _estimate_distinct as est

    m, n = 1 << 18, 45_000_000
    assert est(2, m, n) < 100
    assert 3 * 3500 <= est(3500, m, n) < 12_000            # stays on the LDS-table path
    assert est(20_000, m, n) > 11_000                       # partitioned path
    assert est(m - 10, m, n) == n                           # (almost) all unique
    for D in (50_000, 1_000_000, 20_000_000):               # uniform model, within the 3x margin
        d = int(D * (1 - np.exp(-m / D)))
        assert D <= est(d, m, n) <= min(n, 3.5 * D + 100)


def test_rank_sharding_semantics(tmp_path):
    """Under torch.distributed a parquet dataset is a global list (rank r takes every world-th
    partition); frames handed over in memory are the rank's own shard and are all kept --
    bench.py builds one frame per rank, which an index filter would silently drop on ranks > 0."""
    import pandas as pd

    from nvtabular_amd.io import Dataset

    parts = [pd.DataFrame({"a": np.arange(4) + 10 * i}) for i in range(5)]
    mem = Dataset(parts)
    assert len(list(mem._host_parts(None, None))) == 5
    assert len(list(mem._host_parts(None, (1, 2)))) == 5      # rank-local: nothing is skipped
    one = Dataset(parts[0])
    assert len(list(one._host_parts(None, (3, 8)))) == 1       # the bench.py case
    path = tmp_path / "d.parquet"
    pd.concat(parts).to_parquet(path, row_group_size=4)
    pq = Dataset(str(path), engine="parquet", row_groups_per_part=1)
    assert pq.npartitions == 5

    def first(t):   # (a pyarrow table, or the hand-written reader's staged partition)
        return int(t.columns["a"].values[0]) if hasattr(t, "to_device") else t.column("a")[0].as_py()

    firsts = lambda shard: [first(t) for t in pq._host_parts(None, shard)]
    assert firsts(None) == [0, 10, 20, 30, 40]
    assert firsts((0, 2)) == [0, 20, 40] and firsts((1, 2)) == [10, 30]


def test_path_selection_thresholds():
    """kernels._path_for: the C-ABI path id for an expected distinct count (include/nvt_hip.h)."""
    from nvtabular_amd import kernels as K

    assert K._path_for(0) == 0                      # unknown: start on the plain LDS-table path
    assert K._path_for(3) == 6 and K._path_for(64) == 6
    assert K._path_for(65) == 0 and K._path_for(K.PATH_S_MAX_DISTINCT) == 0
    # 11-21 k keys: two key classes (path 7) only for int64 keys / weighted merges
    # int32 keys without weights: the range path (9) from the end of the LDS-table path up to
    # ~6.5 M distinct keys, hash partitions beyond
    assert K._path_for(K.PATH_S_MAX_DISTINCT + 1) == 9
    assert K._path_for(int(K.PATH_S2_FACTOR * K.PATH_S_MAX_DISTINCT) + 1) == 9
    assert K._path_for(K.PATH_P1_MAX_DISTINCT + 1) == 9
    # beyond the range path: the sort path (int32 keys without weights), hash partitions otherwise
    assert K._path_for(K.PATH_RANGE_MAX_DISTINCT + 1) == K.PATH_SORT
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1) == K.PATH_SORT
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1, small_tables=True) == 3
    j = K.DenseCountJob.__new__(K.DenseCountJob)
    j.min_range_bits = 8
    # (round 6: 10000 keys per bucket -- 256 buckets up to 2.56 M keys, 512 up to 5.12 M)
    kpb = K.RANGE_KEYS_PER_BUCKET
    for hint, bits in ((12_000, 8), (256 * kpb, 8), (256 * kpb + 1, 9), (512 * kpb, 9), (512 * kpb + 1, 10),
                       (6_400_000, 10 if 6_400_000 > 512 * kpb else 9)):
        j.hint = hint
        assert j.range_bits() == bits, (hint, j.range_bits())
    # (int32 keys without weights never reach the global-table fallback: the sort path has no
    # capacity limit below 2^30 rows)
    assert K._path_for(K.PATH_P3_MAX_DISTINCT + 1) == K.PATH_SORT
    assert K._path_for(K.PATH_P3_MAX_DISTINCT + 1, small_tables=True) == -1   # global-table fallback
    # int64 keys / weighted merges use the smaller tables
    assert K._path_for(K.PATH_S_MAX_WEIGHTED + 1, small_tables=True) == 7
    assert K._path_for(int(K.PATH_S2_FACTOR * K.PATH_S_MAX_WEIGHTED) + 1, small_tables=True) == 1
    assert K._path_for(K.PATH_P1_MAX_SMALL + 1, small_tables=True) == 2
    assert K._path_for(K.PATH_P2_MAX_DISTINCT + 1, small_tables=True) == 3
    # escalation order covers every automatic path exactly once
    assert sorted(K.PATH_ORDER) == [0, 1, 2, 3, 6, 7] and set(K._path_max()) >= set(K.PATH_ORDER)


def test_encode_kind_and_launch_shape_tables():
    """kernels_encode.encode_kind / encode_launch_shape: the kind of table a vocabulary gets and the
    kernel it is encoded with, as literal tables (csrc/nvt_encode.hip: enc_shape_of decides the
    second one again, under the same names)."""
    from nvtabular_amd import kernels as K

    # (key_bytes, n_vocab, unique, defer_build, has_range_table, flat) -> kind
    kinds = [
        ((4, 5000, True, False, False, False), "resident"),
        ((4, 100_000, True, True, True, False), "dumped"),
        ((4, 100_000, True, True, False, True), "flat"),
        ((4, 100_000, True, False, False, False), "cache"),
        ((4, 100_000, True, True, False, False), "cache"),
        ((8, 100_000, True, False, False, False), "linear64"),
        ((4, 100_000, False, False, False, False), "generic"),
        # the resident boundary
        ((4, 1, True, False, False, False), "resident"), ((4, 8192, True, False, False, False), "resident"),
        ((4, 8193, True, False, False, False), "cache"),
        ((8, 6144, True, False, False, False), "resident"), ((8, 6145, True, False, False, False), "linear64"),
        ((8, 8192, True, True, False, False), "linear64"),
        # no keys: a hashed table with nothing in it, whatever else was asked for
        ((4, 0, True, False, False, False), "generic"), ((8, 0, True, True, False, False), "generic"),
        ((4, 0, False, False, False, False), "generic"),
        # duplicate keys: never staged in LDS, however few
        ((4, 10, False, False, False, False), "generic"), ((8, 6144, False, False, False, False), "generic"),
        ((4, 100_000, False, True, False, True), "generic"),
        # a range table or flat offered to a vocabulary that fits LDS: still resident
        ((4, 8192, True, True, True, False), "resident"), ((4, 4097, True, True, False, True), "resident"),
        ((4, 8193, True, True, True, False), "dumped"), ((4, 8193, True, True, False, True), "flat"),
        # flat needs defer_build and int32 keys
        ((4, 100_000, True, False, False, True), "cache"), ((8, 100_000, True, True, False, True), "linear64"),
    ]
    for args, kind in kinds:
        assert K.encode_kind(*args) == kind, (args, kind)
    for bad in ((4, 100_000, True, False, True, False), (4, 100_000, False, True, True, False),
                (8, 100_000, True, True, True, False)):
        try:
            K.encode_kind(*bad)
        except AssertionError:
            continue
        raise AssertionError(f"a range table was accepted for {bad}")

    small, wide = "encode_small_kernel<2048>", "encode_small_kernel<4096>"
    hot = "encode_hot_kernel<GLOBAL=false>"
    # (kind, key_bytes, out_bytes, n_vocab, has_head_image) -> launch shape
    shapes = [
        (("generic", 4, 8, 100_000, False), "encode_kernel"), (("generic", 8, 4, 0, False), "encode_kernel"),
        (("resident", 4, 8, 1, False), small), (("resident", 4, 8, 1024, False), small),
        (("resident", 4, 8, 1025, False), wide), (("resident", 4, 8, 2048, False), wide),
        (("resident", 4, 8, 2049, False), hot), (("resident", 4, 8, 8192, False), hot),
        (("resident", 4, 4, 1024, False), hot), (("resident", 4, 4, 1025, False), hot),
        (("resident", 4, 4, 2048, False), hot), (("resident", 4, 4, 2049, False), hot),
        (("resident", 8, 8, 1024, False), hot), (("resident", 8, 4, 2048, False), hot),
        (("resident", 8, 8, 6144, False), hot),
        (("linear64", 8, 8, 6145, False), "encode_hot_kernel<int64,GLOBAL=true>"),
        (("linear64", 8, 4, 100_000, False), "encode_hot_kernel<int64,GLOBAL=true>"),
        (("cache", 4, 8, 8193, True), "cache mode, head image"),
        (("cache", 4, 4, 8193, False), "cache mode, head per launch"),
        (("flat", 4, 8, 100_000, True), "encode_pipe_kernel<2>"), (("flat", 4, 4, 100_000, False), "encode_pipe_kernel<2>"),
        (("dumped", 4, 8, 100_000, True), "encode_pipe_kernel<1>"),
        (("dumped", 4, 4, 100_000, False), "encode_pipe_kernel<1>"),
    ]
    for args, shape in shapes:
        assert K.encode_launch_shape(*args) == shape, (args, shape)


def test_count_escalation_replays_the_recorded_grid():
    """kernels_count.escalate + _launch_path_of against tests/golden/count_escalation_v1.json: what
    DenseCountJob.resolve did with every overflow word before the policy became a pure function
    (grid and origin: profiles/count_driver_notes.md).  Every row, every field."""
    import json
    import os

    from nvtabular_amd import _lib, kernels as K
    from nvtabular_amd.kernels_count import DONE, FALLBACK

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count_escalation_v1.json")) as f:
        doc = json.load(f)
    fields = doc["fields"]
    assert fields[:-2] == list(K.CountPolicy._fields) and fields[-2:] == ["ovf", "need"]
    assert doc["outcome"] == ["verdict", "path", "cap_guess", "min_range_bits", "range_failed",
                              "range_fail_bits", "launch"]
    assert len(doc["rows"]) > 2000
    for row in doc["rows"]:
        args = dict(zip(fields, row))
        ovf, need = args.pop("ovf"), args.pop("need")
        args["pieces"] = object() if args["pieces"] else None
        try:
            nxt = K.escalate(K.CountPolicy(**args), ovf, need)
        except _lib.NvtHipError as e:
            got = ["error: " + str(e)] + [None] * 6
        else:
            assert nxt is not DONE, row
            got = ["fallback"] + [None] * 6 if nxt is FALLBACK else [
                "relaunch", nxt.path, nxt.cap_guess, nxt.min_range_bits, nxt.range_failed,
                nxt.range_fail_bits, K._launch_path_of(nxt, nxt.path)]
        assert got == row[len(fields):], (row, got)
    assert K.escalate(K.CountPolicy(path=9, kb=4, weighted=False, hint=0, n=10), 0, 0) is DONE


def test_count_stream_assignment():
    """kernels_count.assign_streams: launch order and workspace slot per column.  The expected
    values are what the loop inside CountBatch._launch produced for these inputs before it was
    lifted out (profiles/count_driver_notes.md)."""
    from nvtabular_amd import kernels as K

    paths = [9, 9, 0, 6, 9, 0, 7]
    ns = [4_000_000, 1_000_000, 3_000_000, 500_000, 2_500_000, 3_500_000, 700_000]
    cases = [
        (paths, ns, 1, True, [0, 1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 0, 0]),
        # (the LDS-resident columns go first; an LDS-resident LAST column takes the head start away)
        (paths, ns, 3, True, [2, 3, 5, 0, 1, 4, 6], [2, 1, 2, 0, 2, 1, 1]),
        (paths, ns, 3, False, [0, 1, 2, 3, 4, 5, 6], [0, 2, 2, 1, 1, 2, 1]),
        # two LDS-resident columns for three streams: they go first, without a head start
        ([9, 0, 9, 6, 1], [900, 800, 700, 600, 500], 3, True, [1, 3, 0, 2, 4], [2, 1, 0, 1, 2]),
        ([0, 6, 7], [100, 200, 300], 3, True, [0, 1, 2], [2, 1, 0]),          # nothing to run ahead of
        ([9], [1000], 3, True, [0], [0]),
        ([10, 9, 0, 6], [5000, 4000, 3000, 2000], 2, True, [2, 3, 0, 1], [0, 1, 1, 0]),
        ([0, 0, 0, 9, 0], [500, 400, 300, 200, 100], 3, True, [0, 1, 2, 3, 4], [1, 2, 2, 0, 1]),
        # a head start: three LDS-resident columns, one stream each whatever their cost
        (paths + [9], ns + [2_000_000], 3, True, [2, 3, 5, 0, 1, 4, 6, 7], [0, 1, 2, 1, 2, 0, 0, 2]),
        (paths + [9], ns + [2_000_000], 3, False, [0, 1, 2, 3, 4, 5, 6, 7], [0, 2, 1, 0, 1, 2, 1, 2]),
    ]
    for p, n, streams, head_start, order, slots in cases:
        got_order, got_slots = K.assign_streams(p, n, streams, head_start)
        assert (list(got_order), list(got_slots)) == (order, slots), (p, streams, head_start)
        assert sorted(got_order) == list(range(len(p))) and len(got_slots) == len(p)
        assert all(0 <= k < streams for k in got_slots)
    order, slots = K.assign_streams(paths + [9], ns + [2_000_000], 3, True)
    assert all(paths[i] in (0, 6, 7) for i in order[:3]) and sorted(slots[:3]) == [0, 1, 2]


def test_count_memory_learn():
    """kernels_count.CountMemory.learn on synthetic info dicts.  (The branch that adopts splitters
    from a sort-path list calls range_splitters, a device function: tests/test_gpu_range_path.py
    covers it.)"""
    import torch

    from nvtabular_amd import kernels as K

    k32 = torch.empty(0, dtype=torch.int32)
    ok = dict(path=K.PATH_RANGE, distinct=100_000, max_count=9, rows=10**6, sorted_by_key=True,
              range_fail_bits=0, range_bits_floor=8, range_pieces=False)
    fail = dict(path=1, distinct=100_000, max_count=9, rows=10**6, range_failed=True, range_fail_bits=33)
    m = K.CountMemory()
    assert m.job_args("c") == dict(hint=0, allow_range=True, pieces=None, min_range_bits=8)
    m.learn("c", k32, None, 0, dict(path=0, distinct=7, max_count=3, rows=50))
    assert m.cap_hints["c"] == 64 and m.last_paths["c"] == 0 and m.range_oks == {}   # max(64, distinct)
    m.learn("c", k32, None, 0, ok)
    assert m.cap_hints["c"] == 100_000 and m.range_oks == {"c": 1} and m.last_paths["c"] == 9
    m.learn("c", k32, None, 0, dict(ok, path=K.PATH_SORT))       # a success counts on path 9 only
    assert m.range_oks == {"c": 1}
    # the bucket floor: only a good hint raises it
    m = K.CountMemory()
    m.learn("c", k32, None, 0, dict(ok, range_bits_floor=10))     # no hint before
    assert m.range_bits_floor == {}
    m.learn("c", k32, None, 0, dict(ok, distinct=125_001, range_bits_floor=10))   # outgrew 100 000 + a quarter
    assert m.range_bits_floor == {}
    m.learn("c", k32, None, 0, dict(ok, distinct=125_001 + 31_250, range_bits_floor=10))   # within a quarter
    assert m.range_bits_floor == {"c": 10} and m.job_args("c")["min_range_bits"] == 10
    # the ban: two overflows that make up more than a fifth of the attempts
    m = K.CountMemory()
    m.learn("c", k32, None, 0, fail)
    assert m.range_failures == [("c", 33, 100_000)] and not m.no_range and m.job_args("c")["allow_range"]
    m.learn("c", k32, None, 0, fail)
    assert m.no_range == {"c"} and not m.job_args("c")["allow_range"]
    m = K.CountMemory()
    m.range_oks["c"] = 8
    m.learn("c", k32, None, 0, fail)
    m.learn("c", k32, None, 0, fail)
    assert len(m.range_failures) == 2 and not m.no_range           # 4 * 2 fails <= 8 successes
    m.learn("d", k32, None, 0, fail)                               # (another column's failures do not count)
    m.range_oks["c"] = 7
    m.learn("c", k32, None, 0, fail)
    assert m.no_range == {"c"}
    # an overflow WITH splitters (sort-path list back): the splitters go, the failure stays
    m = K.CountMemory()
    m.range_pieces["c"] = object()
    m.learn("c", k32, None, 0, dict(fail, path=K.PATH_SORT, sorted_by_key=True, range_pieces=True))
    assert m.range_pieces == {} and m.job_args("c")["pieces"] is None and len(m.range_failures) == 1


def test_shuffle_option_coercion():
    from nvtabular_amd.io import Shuffle

    assert Shuffle.coerce(None) is None and Shuffle.coerce(False) is None
    assert Shuffle.coerce(True) == Shuffle.PER_WORKER
    assert Shuffle.coerce(Shuffle.PER_PARTITION) == Shuffle.PER_PARTITION
    assert Shuffle.coerce(Shuffle.FULL) == Shuffle.PER_WORKER
    import pytest

    with pytest.raises(ValueError):
        Shuffle.coerce("sideways")


def test_graph_json_dtype_and_tag_records():
    """The merlin DType / Tags records of graph_serializer.py:106-153 as this engine writes
    and reads them."""
    from nvtabular_amd import Tags
    from nvtabular_amd import graph_json as G

    d = G._dtype_to_dict(np.dtype("int32"), with_shape=True)
    assert d == {"name": "int32", "element_type": "int", "element_size": 32, "signed": True,
                 "shape": [{"min": None, "max": None}]}
    assert G._dtype_to_dict(np.float64)["element_type"] == "float"
    lst = G._dtype_to_dict(np.int64, is_list=True, is_ragged=True, with_shape=True)
    assert len(lst["shape"]) == 2 and lst["shape"][1] == {"min": 0, "max": None}
    assert G._dtype_from_dict({"name": "int64"}) == np.dtype("int64")
    assert G._dtype_from_dict("float32") == np.dtype("float32")
    assert G._dtype_from_dict({"name": "str"}) == np.dtype("O")
    assert G._dtype_from_dict({"name": "weird", "element_type": "uint", "element_size": 8}) == np.dtype("uint8")
    assert G._tags_to_list([Tags.CATEGORICAL, Tags.LIST]) == ["Tags.CATEGORICAL", "Tags.LIST"]
    assert G._tags_from_list(["Tags.CONTINUOUS", "categorical", "Tags.NOT_A_TAG"]) == [
        Tags.CONTINUOUS, Tags.CATEGORICAL]
    assert G._paths_from_json(G._paths_to_json({("a", "b"): "/x/art/categories/u.parquet"}, "/x/art"),
                              "/y") == {("a", "b"): "/y/categories/u.parquet"}


def test_one_pass_class_order_equals_count_desc_key_asc():
    """The rule behind nvt_vocab_order.hip's cls_scatter_kernel, emulated in numpy: for a KEY-SORTED
    (key, count) list, "count descending, key ascending" (categorify.py:1300,1316 with the stable
    tie rule) == class 255 (count >= 255) sorted on its own, followed by classes 254 .. 1, each in
    the key order the list already has.  (The GPU tests compare the kernel with the oracle; this
    pins the algebra the kernel relies on.)"""
    import numpy as np

    rng = np.random.default_rng(0)
    keys = np.unique(rng.integers(-2**31, 2**31 - 1, 50_000).astype(np.int64))  # sorted, distinct
    counts = np.minimum(rng.zipf(1.3, keys.size), 10**6).astype(np.int64)
    want = np.lexsort((keys, -counts))                       # count desc, key asc
    cls = np.minimum(counts, 255)
    digit = 255 - cls                                        # class 255 first
    order = np.argsort(digit, kind="stable")                 # ONE stable counting pass
    n_big = int((cls == 255).sum())
    head = order[:n_big]
    head = head[np.lexsort((keys[head], -counts[head]))]     # the small sort of class 255
    got = np.concatenate([head, order[n_big:]])
    np.testing.assert_array_equal(got, want)
    # and the flat range table: positions of the sorted keys under a monotone slot function with
    # linear probing are a prefix maximum, p_i = i + max_{j <= i}(h_j - j)
    slots = 1 << 17
    span = int(keys[-1] - keys[0])
    h = ((keys - keys[0]).astype(np.float64) * (slots / (span + 1))).astype(np.int64)
    p = np.arange(keys.size) + np.maximum.accumulate(h - np.arange(keys.size))
    ref = np.empty(keys.size, dtype=np.int64)
    last = -1
    for i, hi in enumerate(h.tolist()):                      # sequential linear probing
        last = max(hi, last + 1)
        ref[i] = last
    np.testing.assert_array_equal(p, ref)


def test_fold_sparse_and_sorted_groupby_eligibility():
    """Host logic of the groupby sort path: dense per-(group, fold) statistics -> the compacted
    [fold, key] groups of the reference's second aggregate (only pairs that have rows), and
    which inputs may take the sort path at all."""
    import torch

    from nvtabular_amd import kernels as K
    from nvtabular_amd.ops._groupby import fold_sparse

    kfold = 3
    keys = torch.tensor([-7, 2, 40], dtype=torch.int64)
    fsize = torch.tensor([1, 0, 2, 0, 0, 5, 3, 3, 0], dtype=torch.int64)  # [g * kfold + f]
    fsum = torch.arange(9, dtype=torch.float64) * 1.5
    comp = dict(keys=[keys], n=3, fold=dict(kfold=kfold, size=fsize, sum=[fsum]))
    sp = fold_sparse(comp)
    assert sp["n"] == 5
    assert sp["keys"][0].tolist() == [0, 2, 2, 0, 1]          # fold ids
    assert sp["keys"][1].tolist() == [-7, -7, 2, 40, 40]      # keys
    assert sp["size"].tolist() == [1, 2, 5, 3, 3] and sp["count"].tolist() == sp["size"].tolist()
    assert sp["sum"][0].tolist() == [0.0, 3.0, 7.5, 9.0, 10.5]
    assert sp["null_mask"].tolist() == [0] * 5 and sp["sumsq"] == [] and sp["min"] == []
    n = K.SORTED_GROUPBY_MIN_ROWS
    k32, k64 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    assert K.sorted_groupby_eligible(k32, None, n) and K.sorted_groupby_eligible(k64, None, n, 5)
    assert not K.sorted_groupby_eligible(k32, None, n - 1)                 # launch latency
    assert not K.sorted_groupby_eligible(k32, torch.zeros(1, dtype=torch.uint8), n)  # null keys
    assert not K.sorted_groupby_eligible(torch.zeros(4, dtype=torch.uint8), None, n)
    assert not K.sorted_groupby_eligible(k32, None, n, K.SORTED_GROUPBY_MAX_KFOLD + 1)
    assert not K.sorted_groupby_eligible(k32, None, (1 << 29) + 1, 5)      # row index + 3 fold bits > 32
    assert K.sorted_groupby_eligible(k32, None, (1 << 29), 5)


def test_harness_rehearsals_collect_last():
    """Tests that shell out to bench.py / torchrun live in test_zz_rehearsals.py only: under
    `pytest -x` a harness assertion must not be able to mask the kernel-parity tests collected
    behind it (Weak #1)."""
    import glob
    import os
    import re

    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "test_*.py")))
    assert os.path.basename(files[-1]) == "test_zz_rehearsals.py"
    for f in files[:-1]:
        if os.path.basename(f).startswith("test_gpu_"):
            src = open(f).read()
            assert not re.search(r"subprocess|torch\.distributed\.run", src), f


def test_bench_parity_verdicts_cover_every_leg():
    """bench.parity_verdicts: a failed nested leg, an extra that died and an extra without a parity leg
    all make the line's top-level verdict false; only oracle legs count into parity_rows."""
    import bench

    line = {"parity": {"parity_checked_rows": 100, "parity_ok": True, "full_frame_ok": True},
            "extra_configs": {"a": {"parity": {"method": "oracle ...", "parity_checked_rows": 5, "parity_ok": True}},
                              "b": {"parity": {"method": "files ...", "files_equal_in_memory_transform": True}},
                              "c": {"parity": {"method": "properties ...", "parity_ok": True, "rows": 10 ** 9}}}}
    assert bench.parity_verdicts(line) == (True, 105, [])
    line["parity"]["full_frame_ok"] = False
    line["extra_configs"]["a"]["parity"]["parity_ok"] = False
    line["extra_configs"]["d"] = {"error": "RuntimeError('x')"}
    line["extra_configs"]["e"] = {"ms_per_step": 1.0}
    ok, rows, failed = bench.parity_verdicts(line)
    assert not ok and failed == ["headline.full_frame", "a", "d:error", "e:no parity leg"]
