"""The counting driver of Categorify.fit: nvt_count_* (global tables), nvt_dense_count_many (dense
(key, count) lists), the policy that picks a column's path and escalates it after an overflow,
and what the driver remembers about a column between partitions (CountMemory).

The policy is pure: ``_path_for`` (first path), ``escalate`` (next state after an overflow),
``_launch_path_of`` (the path word of the C call) and ``assign_streams`` (launch order and
workspace slots) touch neither torch nor the library, and tests/test_host_logic.py pins them.

Part of the host driver of the C ABI (include/nvt_hip.h); ``kernels.py`` is the facade every
caller imports -- it re-exports these names, holds the run-time switches they read (``K.<FLAG>`` at
call time: tests and A / B runs set them on the facade) and the helpers they share."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from . import kernels as K
from ._lib import check

MIN_COUNT_CAPACITY = 1 << 16


# --------------------------------------------------------------------------
# Categorify.fit: count tables
# --------------------------------------------------------------------------
class CountTable:
    """Open-addressing (key -> count) table in HBM for one column (group)."""

    def __init__(self, key_dtype: torch.dtype, capacity: int, device=None):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.key_dtype = key_dtype
        self.key_bytes = 4 if key_dtype == torch.int32 else 8
        self.suffix = "i32" if self.key_bytes == 4 else "i64"
        self.capacity = K.next_pow2(capacity)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        nbytes = C.c_uint64()
        check(self.lib.nvt_count_table_bytes(self.key_bytes, self.capacity, C.byref(nbytes)))
        self.table = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.state = torch.zeros(_lib.STATE_WORDS, dtype=torch.int64, device=self.device)
        self.clear()

    def clear(self):
        with K._timed("count_clear", 0):
            check(
                self.lib.nvt_count_clear(
                    self.table.data_ptr(), self.key_bytes, self.capacity, self.state.data_ptr(),
                    K.stream_ptr(),
                ),
                "nvt_count_clear",
            )

    def update(self, keys: torch.Tensor, valid: Optional[torch.Tensor]):
        assert keys.dtype == self.key_dtype
        keys = K.aligned(keys)
        fn = getattr(self.lib, f"nvt_count_{self.suffix}")
        with K._timed(f"count_{self.suffix}", keys.numel() * self.key_bytes):
            check(
                fn(keys.data_ptr(), K.ptr(valid), keys.numel(), self.table.data_ptr(),
                   self.capacity, self.state.data_ptr(), K.stream_ptr()),
                f"nvt_count_{self.suffix}",
            )

    def merge(self, keys: torch.Tensor, counts: torch.Tensor):
        assert keys.dtype == self.key_dtype and counts.dtype == torch.int64
        fn = getattr(self.lib, f"nvt_count_merge_{self.suffix}")
        check(
            fn(keys.contiguous().data_ptr(), counts.contiguous().data_ptr(), keys.numel(),
               self.table.data_ptr(), self.capacity, self.state.data_ptr(), K.stream_ptr()),
            f"nvt_count_merge_{self.suffix}",
        )

    def read_state(self) -> List[int]:
        return self.state.cpu().tolist()  # synchronises the stream

    def compact(self, occupied: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Dense (keys, counts[int64]) in arbitrary order, sentinel-key rows included."""
        st = self.read_state()
        occ = st[_lib.ST_OCCUPIED] if occupied is None else occupied
        out_k = torch.empty(occ + 1, dtype=self.key_dtype, device=self.device)
        out_c = torch.empty(occ + 1, dtype=torch.int64, device=self.device)
        out_n = torch.zeros(1, dtype=torch.int64, device=self.device)
        fn = getattr(self.lib, f"nvt_count_compact_{self.suffix}")
        with K._timed("count_compact", 0):
            check(
                fn(self.table.data_ptr(), self.capacity, out_k.data_ptr(), out_c.data_ptr(),
                   out_n.data_ptr(), K.stream_ptr()),
                f"nvt_count_compact_{self.suffix}",
            )
        n = occ
        if st[_lib.ST_SENTINEL] > 0:
            # rows whose key equals the empty-slot sentinel are counted on the side
            out_k[n] = K.INT32_MIN if self.key_bytes == 4 else K.INT64_MIN
            out_c[n] = st[_lib.ST_SENTINEL]
            n += 1
        return out_k[:n], out_c[:n]


def count_into_new_table(
    keys_list: Sequence[torch.Tensor],
    valid_list: Sequence[Optional[torch.Tensor]],
    hint: int,
    max_tries: int = 8,
) -> Tuple[CountTable, List[int]]:
    """Groupby-size of one partition's column(s) into a fresh table sized from
    ``hint`` (expected distinct keys); regrows and recounts on overflow, which
    is safe because the table only holds this partition."""
    total = sum(int(k.numel()) for k in keys_list)
    # never below 2^16 slots: a tiny table puts every block's end-of-kernel flush on the
    # same few memory channels (measured: 36 keys in a 128-slot table cost 340 us of
    # serialised atomics; spread over 512 KiB they cost ~10 us)
    cap = K.next_pow2(max(MIN_COUNT_CAPACITY, 2 * min(max(hint, 32), max(total, 32))))
    for _ in range(max_tries):
        tab = CountTable(keys_list[0].dtype, cap)
        for k, v in zip(keys_list, valid_list):
            tab.update(k, v)
        st = tab.read_state()
        if not st[_lib.ST_OVERFLOW] and st[_lib.ST_OCCUPIED] * 10 <= tab.capacity * 7:
            return tab, st
        cap = K.next_pow2(max(16 * cap, 3 * st[_lib.ST_OCCUPIED]))
    raise _lib.NvtHipError("count table kept overflowing; cardinality estimate diverged")


# --------------------------------------------------------------------------
# Categorify.fit, atomic-free: dense (key, count) lists
# --------------------------------------------------------------------------
PATH_S_MAX_DISTINCT = int(os.environ.get("NVT_S_MAX", 11000))          # path 0 (int32 keys, unweighted): 16384-slot LDS tables
PATH_S_MAX_WEIGHTED = 5000          # path 0 for weighted merges / int64 keys: 8192 slots
# Path 7 = path 0 with 2 key classes per row slab (column read twice): 350 us against 420 us on
# path 1 for 12-21 k distinct keys.
# escalation order when a path's LDS tables overflow (C-ABI path ids, include/nvt_hip.h)
PATH_ORDER = [6, 0, 7, 1, 2, 3]
_S_CLASSES = {6: 1, 0: 1, 7: 2}
PATH_S2_FACTOR = 1.95               # path 7: path 0 with 2 key classes per row slab (column read twice)
# (K.PATH_TINY_MAX = 64: path 6, path 0 with hot keys replicated per lane group)
PATH_P1_MAX_DISTINCT = int(os.environ.get("NVT_P1_MAX", 2_400_000))    # path 1: ONE level, 256 buckets x 16384-slot tables (int32)
PATH_P1_MAX_SMALL = 1_100_000       #         ... 8192-slot tables (int64 keys / weighted merges)
PATH_P2_MAX_DISTINCT = 9_000_000    # path 2: 64 x 64 buckets, 4096-slot tables
PATH_P2_MAX_WEIGHTED = 18_000_000   #         weighted: 8192-slot tables
# path 3: 64 x 256 = 16384 buckets, 8192-slot tables that may fill to 6144: at 60 M distinct keys a
# bucket holds 3662 +- 60 of them (Poisson), 40 % headroom -- Criteo-1TB's largest columns
# (C1 / C10 / C20 / C22: 38.5-40.0 M uniques, dask-nvtabular-criteo-benchmark.py:360-366) stay on
# the atomic-free path whether they arrive as one partition or as a merge of partial lists
PATH_P3_MAX_DISTINCT = 60_000_000

# path 9 (range path, include/nvt_hip.h NVT_PATH_RANGE): int32 keys without weights up to
# K.PATH_RANGE_MAX_DISTINCT distinct keys; ONE partition pass by key range + per-bucket tables
# emitted in key order.  Buckets are sized for <= ~5000 distinct keys (16384-slot tables addressed
# by a monotone function of the key want a low load).
PATH_RANGE = 9
PATH_PIECES = 0x10000   # include/nvt_hip.h NVT_PATH_PIECES
RANGE_AUX_WORDS, RANGE_AUX_HIST, RANGE_AUX_PW = 13600 + 256, 8208, 13600   # include/nvt_hip.h NVT_RANGE_AUX_*
# distinct keys per bucket the bucket count (256 / 512 / 1024) is chosen for.  Round 6: 10000 (load
# 0.61 of the 16384-slot tables) instead of 5000: fewer bins in the partition pass and range tables
# of half the size -- count 3.90 -> 3.66 ms, ordering 0.87 -> 0.76 ms on cfg2.  A bucket holds at
# most 12288 keys (NVT_OVF_FULL); a column whose keys are not spread evenly enough for that is
# relaunched with all 1024 buckets and REMEMBERED (info["range_bits_floor"] -> CountMemory).
RANGE_KEYS_PER_BUCKET = int(os.environ.get("NVT_RANGE_KEYS_PER_BUCKET", "10000"))

# path 10 (sort path, NVT_PATH_SORT): int32 keys without weights beyond the range path -- radix sort
# of the rows + run lengths, key-sorted output (Criteo-1TB's 38-40 M-unique columns)
PATH_SORT = 10

_ws_cache = {}
_RT_BYTES = {}   # range_bits -> nvt_range_table_bytes
_WS_BYTES = {}   # (key_bytes, n, path, weighted) -> nvt_dense_count_ws_bytes

PATH_HOT, HOT_IMAGE_WORDS = 16, 8192   # include/nvt_hip.h NVT_PATH_HOT, NVT_HOT_IMAGE_WORDS
_PATH_COST = {6: 0.5, 0: 0.7, 7: 1.7, 9: 2.0, 1: 2.5, 2: 3.2, 3: 3.5, 10: 6.0}

SAMPLE_ROWS = 1 << 18               # cold start: distinct keys of this many leading rows ...
SAMPLE_MIN_ROWS = 8 * SAMPLE_ROWS   # ... when the column is at least this long


def _workspace(nbytes: int, device, slot: int = 0) -> torch.Tensor:
    key = (device.type, device.index, slot)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _ws_cache.pop(key, None)
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# --------------------------------------------------------------------------
# the policy: no torch, no ctypes
# --------------------------------------------------------------------------
def _path_for(hint: int, small_tables: bool = False, allow_range: bool = True) -> int:
    """First path of a column expected to hold ``hint`` distinct keys (0: unknown).
    small_tables: int64 keys or a weighted merge."""
    s_max = PATH_S_MAX_WEIGHTED if small_tables else PATH_S_MAX_DISTINCT
    if 0 < hint <= K.PATH_TINY_MAX:
        return 6
    if hint <= s_max:
        return 0
    if small_tables:
        if hint <= PATH_S2_FACTOR * s_max:
            return 7  # (int32 keys: the filtered path 1 is faster there, 241 against 307 us)
        if hint <= PATH_P1_MAX_SMALL:
            return 1
        if hint <= PATH_P2_MAX_DISTINCT:
            return 2
        return 3 if hint <= PATH_P3_MAX_DISTINCT else -1   # (-1: global-table fallback)
    if allow_range and hint <= K.PATH_RANGE_MAX_DISTINCT:
        return PATH_RANGE
    # more keys than the range path holds, or a column the range path gave up on (keys that
    # cluster in their range): the sort path keeps its per-partition lists KEY-ORDERED, which is
    # what the partition merge and the one-pass vocabulary ordering live on; the hash paths would
    # hand back unordered lists
    return PATH_SORT


def _path_max() -> dict:
    """Distinct keys each path is sized for: the output-capacity guess when a path is entered by
    escalation."""
    return {6: 1024, 0: 98304, 7: 196608, 9: K.PATH_RANGE_MAX_DISTINCT, 10: 1 << 30,
            1: PATH_P1_MAX_DISTINCT, 2: PATH_P2_MAX_DISTINCT, 3: PATH_P3_MAX_DISTINCT}


class CountPolicy(NamedTuple):
    """What the policy reads of a DenseCountJob (the job itself has the same attributes)."""
    path: int
    kb: int                        # key bytes
    weighted: bool
    hint: int
    n: int
    allow_range: bool = True       # False: the range path overflowed on this column before
    range_failed: bool = False     # ... in this very call
    range_fail_bits: int = 0       # NVT_OVF_*: region / probe / full of the first such overflow
    min_range_bits: int = 8
    cap_guess: int = 1 << 16       # entries of the output list
    hot: Optional[bool] = None     # None: hot-key filter when eligible; True / False: forced
    pieces: object = None          # splitters of the piecewise range map, or None


DONE, FALLBACK = "done", "global-table fallback"


def _range_bits(s) -> int:
    """log2 of the bucket count of the range path: 256 .. 1024 buckets."""
    want = max(1, -(-max(s.hint, 1) // RANGE_KEYS_PER_BUCKET))
    return max(s.min_range_bits, min(10, max(8, (want - 1).bit_length())))


def _launch_path_of(s, path: int) -> int:
    """The `path` argument of the C call: partitioned paths of int32 keys without weights get
    the hot-key filter in front (include/nvt_hip.h, NVT_PATH_HOT)."""
    if path == PATH_RANGE:
        return PATH_RANGE | (_range_bits(s) << 8) | (PATH_PIECES if s.pieces is not None else 0)
    eligible = path in (1, 2, 3) and s.kb == 4 and not s.weighted
    return path | PATH_HOT if eligible and (s.hot is None or s.hot) else path


def escalate(s: CountPolicy, ovf: int, need: int):
    """What follows from the overflow word and ST_NEED a job read back: DONE, FALLBACK (the
    global table) or the state to relaunch with; raises where no relaunch can help."""
    if ovf & 1:   # LDS tables
        if s.path == PATH_SORT:  # (no LDS tables to overflow)
            raise _lib.NvtHipError("dense count: the sort path reported a table overflow")
        int32_plain = s.kb == 4 and not s.weighted
        if s.path == PATH_RANGE:
            if _range_bits(s) < 10:
                # more distinct keys than the hint promised (cold start): all 1024 buckets first
                return s._replace(min_range_bits=10, cap_guess=max(s.cap_guess, 1 << 22))
            # (the range path assumes keys spread over their range; a hash path does not)
            if not s.range_failed:
                s = s._replace(range_failed=True, range_fail_bits=int(ovf))
            nxt = 1
        elif s.path == 0 and s.allow_range and int32_plain and not s.range_failed:
            # LDS tables too small: the range path comes next for int32 keys
            return s._replace(path=PATH_RANGE, cap_guess=max(s.cap_guess, 1 << 20))
        elif s.path == PATH_ORDER[-1]:
            return FALLBACK
        else:
            nxt = PATH_ORDER[PATH_ORDER.index(s.path) + 1]
        if nxt == 7 and _launch_path_of(s, 1) & PATH_HOT:
            nxt = 1  # the filtered path 1 beats two key classes (see _path_for)
        if nxt == 1 and s.range_failed and int32_plain:
            # the range path gave up at 1024 buckets: more keys than it holds, or keys that
            # are not spread over their range -- the sort path copes with both in one go
            # (the next fit picks its path from the distinct count found here)
            nxt = PATH_SORT
        elif nxt == 1 and s.hint > PATH_P1_MAX_DISTINCT:
            nxt = 2 if s.hint <= PATH_P2_MAX_DISTINCT else 3
        return s._replace(path=nxt, cap_guess=max(s.cap_guess, _path_max()[nxt]))
    if ovf & 2:   # output list
        if s.cap_guess > s.n:
            raise _lib.NvtHipError("dense count: output list overflowed at full capacity")
        # (the range and sort paths report the exact size; the hash paths only that it was too small)
        exact = need if s.path in (PATH_RANGE, PATH_SORT) else 0
        return s._replace(cap_guess=exact + 64 if exact > s.cap_guess else max(4 * s.cap_guess, 1 << 20))
    return DONE


def assign_streams(paths, ns, streams: int, head_start: bool):
    """(order, slots) of one nvt_dense_count_many call: ``order[k]`` = the pending job launched
    k-th, ``slots[k]`` = its workspace (= internal stream).

    The C call launches the columns in the order of the descriptors, each on the stream of its
    workspace, and a stream waits for the hot-key samples in front of its first FILTERED column.
    In column order every stream began with a range-path column: 243 CUs idled for the ~110 us
    of the sample launch.  With a head start, ``streams`` columns that need no sample
    (LDS-resident: paths 0 / 6 / 7) go first, one per stream whatever their cost, and run under
    the sample; fewer than ``streams`` of them still go first but get no stream of their own, and
    neither do they when the last column is LDS-resident too.  Everything else:
    longest-processing-time assignment."""
    m = len(paths)
    order = list(range(m))
    if streams == 1 or m < 2:
        return order, [0] * m   # shared workspace: the columns are ordered on one stream
    head = 0
    if head_start:
        free = [i for i in order if paths[i] in _S_CLASSES][:streams]
        if free and len(free) < m:
            order = free + [i for i in order if i not in free]
            if len(free) == streams and paths[order[-1]] not in _S_CLASSES:
                head = streams
    cost = [_PATH_COST.get(paths[i], 1.0) * ns[i] for i in order]
    slots, load = list(range(head)) + [0] * (m - head), [0.0] * streams
    for k in range(head):
        load[k] += cost[k]
    for k in sorted(range(head, m), key=lambda k: -cost[k]):
        slots[k] = load.index(min(load))
        load[slots[k]] += cost[k]
    return order, slots


# --------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------
def _plain_info(path: int, distinct: int, max_count: int, rows: int) -> dict:
    return dict(path=path, distinct=distinct, max_count=max_count, rows=rows)


def _empty_result(keys: torch.Tensor):
    """The result of a column without rows."""
    return (torch.empty(0, dtype=keys.dtype, device=keys.device),
            torch.empty(0, dtype=torch.int64, device=keys.device), 0, _plain_info(0, 0, 0, 0))


class DenseCountJob:
    """One column's groupby-size, launched asynchronously; ``dense_count_many`` reads all
    jobs' state words back with a single device->host copy."""

    def __init__(self, keys, valid, weights=None, hint: int = 0, allow_range: bool = True,
                 pieces=None, min_range_bits: int = 8):
        _lib.require_gpu()
        self.want_table = True    # range path: also dump the count tables as the encode table
        self.range_table = None
        self.range_slots = None   # uint32 per entry of the output list: its slot in range_table
        self.allow_range = allow_range
        self.range_failed = False
        self.range_fail_bits = 0
        # range path with a piecewise map (NVT_PATH_PIECES): `pieces` = int32[65] splitters
        # (range_splitters) of a column whose keys are not spread over their range
        self.pieces = pieces
        # (a column that overflowed its buckets in an earlier fit starts with the bucket count
        # that held it: the caller remembers info["range_bits_floor"])
        self.min_range_bits = max(8, min(10, int(min_range_bits)))
        self.lib = _lib.load()
        self.keys = K.aligned(keys)
        self.valid = valid
        self.weights = weights.contiguous() if weights is not None else None
        self.weighted = weights is not None
        self.n = int(self.keys.numel())
        self.dev = self.keys.device
        self.suffix = K._key_suffix(self.keys)
        self.kb = 4 if self.suffix == "i32" else 8
        self.hint = hint
        self.path = _path_for(hint, small_tables=(self.weighted or self.kb == 8),
                              allow_range=allow_range)
        self.cap_guess = max(1 << 16, 2 * max(hint, 1))
        self.state = None  # device uint64[STATE_WORDS] view, assigned by CountBatch
        self.result = None
        self.hot = None    # None: hot-key filter when eligible; True / False: forced (tests, probes)

    def range_bits(self) -> int:
        return _range_bits(self)

    def _policy(self) -> CountPolicy:
        return CountPolicy(*[getattr(self, f) for f in CountPolicy._fields])

    def prepare(self, desc: "_lib.CountCol") -> int:
        """Allocate this attempt's output list and fill one nvt_count_col descriptor; returns
        the workspace bytes the path needs (the caller shares ONE workspace per call)."""
        n, path = self.n, self.path
        out_cap = min(self.cap_guess, n) + 1
        if path in _S_CLASSES:
            # stage 2 has 256 workgroups per key class, each emitting <= 384 keys
            out_cap = min(out_cap, _S_CLASSES[path] * 256 * 384 + 1)
        self.out_k = torch.empty(out_cap + 1, dtype=self.keys.dtype, device=self.dev)
        self.out_c = torch.empty(out_cap + 1, dtype=torch.int64, device=self.dev)
        lpath = _launch_path_of(self, path)
        key = (self.kb, n, lpath, self.weighted)
        nbytes = _WS_BYTES.get(key)
        if nbytes is None:
            out = C.c_uint64()
            check(self.lib.nvt_dense_count_ws_bytes(self.kb, n, lpath, int(self.weighted), C.byref(out)))
            nbytes = _WS_BYTES[key] = out.value
        desc.keys = self.keys.data_ptr()
        desc.valid = K.ptr(self.valid)
        desc.weights = K.ptr(self.weights)
        desc.n = n
        desc.key_bytes = self.kb
        desc.path = lpath
        desc.out_keys = self.out_k.data_ptr()
        desc.out_counts = self.out_c.data_ptr()
        desc.out_capacity = out_cap
        desc.state = self.state.data_ptr()
        desc.hot_image = None
        desc.range_table = desc.out_slots = None
        self.range_slots = None
        if path == PATH_SORT:
            # uint32[256] block that receives the histogram of min(count, 255)
            self.hot_image = torch.empty(256, dtype=torch.int32, device=self.dev)
            desc.hot_image = self.hot_image.data_ptr()
        elif path == PATH_RANGE:
            # aux block: hot image + range parameters (sample kernel) + class histogram
            self.hot_image = torch.empty(RANGE_AUX_WORDS, dtype=torch.int32, device=self.dev)
            if self.pieces is not None:
                self.hot_image[RANGE_AUX_PW:RANGE_AUX_PW + K.RANGE_PIECES + 1] = self.pieces
            desc.hot_image = self.hot_image.data_ptr()
            if self.want_table:
                # the per-bucket count tables, dumped: the column's encode table (range table)
                bits = self.range_bits()
                rt_bytes = _RT_BYTES.get(bits)
                if rt_bytes is None:
                    rt_out = C.c_uint64()
                    check(self.lib.nvt_range_table_bytes(bits, C.byref(rt_out)))
                    rt_bytes = _RT_BYTES[bits] = rt_out.value
                self.range_table = torch.empty(rt_bytes, dtype=torch.uint8, device=self.dev)
                self.table_bits = bits
                desc.range_table = self.range_table.data_ptr()
                # where the dump puts every entry of the list: the ordering labels the table through it
                self.range_slots = torch.empty(out_cap + 1, dtype=torch.int32, device=self.dev)
                desc.out_slots = self.range_slots.data_ptr()
        elif lpath & PATH_HOT:
            # the column's own hot-key table image: sampled for all columns by one launch
            self.hot_image = torch.empty(HOT_IMAGE_WORDS, dtype=torch.int32, device=self.dev)
            desc.hot_image = self.hot_image.data_ptr()
        return nbytes

    def resolve(self, st) -> bool:
        """Inspect the state words read back for this job; False = relaunch needed."""
        ovf = st[_lib.ST_OVERFLOW]
        nxt = escalate(self._policy(), ovf, st[_lib.ST_NEED]) if ovf else DONE
        if nxt is FALLBACK:
            self._fallback()
            return True
        if nxt is not DONE:
            self.path, self.cap_guess, self.min_range_bits = nxt.path, nxt.cap_guess, nxt.min_range_bits
            self.range_failed, self.range_fail_bits = nxt.range_failed, nxt.range_fail_bits
            return False
        m = st[_lib.ST_OCCUPIED]
        max_count = st[_lib.ST_MAXCOUNT]
        if self.path not in (PATH_RANGE, PATH_SORT) and st[_lib.ST_SENTINEL] > 0:
            # (a key-ordered list is already led by the sentinel key, the smallest int32)
            self.out_k[m] = K.INT32_MIN if self.kb == 4 else K.INT64_MIN
            self.out_c[m] = st[_lib.ST_SENTINEL]
            max_count = max(max_count, st[_lib.ST_SENTINEL])
            m += 1
        self.result = (self.out_k[:m], self.out_c[:m], st[_lib.ST_NULLS], self._info(st, m, max_count))
        return True

    def _info(self, st, m: int, max_count: int) -> dict:
        """What the callers learn of a finished attempt.  Categorify tells the paths apart by the
        keys present: ``range_failed`` on every path but the range path, ``sorted_by_key`` and
        what the one-pass vocabulary ordering needs (histogram of min(count, 255), entries >= 255)
        on the range and sort paths, the dumped tables on the range path."""
        info = _plain_info(self.path, m, max_count, st[_lib.ST_ROWS])
        info["range_fail_bits"] = self.range_fail_bits
        if self.path != PATH_RANGE:
            info["range_failed"] = self.range_failed
        if self.path in (PATH_RANGE, PATH_SORT):
            info.update(sorted_by_key=True, cls_hist=self.hot_image, n_big=st[_lib.ST_BIG],
                        range_pieces=self.pieces is not None)
        if self.path == PATH_RANGE:
            info.update(cls_hist=self.hot_image[RANGE_AUX_HIST:RANGE_AUX_HIST + 256],
                        range_aux=self.hot_image, range_table=self.range_table,
                        range_slots=self.range_slots[:m] if self.range_slots is not None else None,
                        range_bits=self.table_bits if self.range_table is not None else 0,
                        range_bits_floor=self.min_range_bits)
        return info

    def _fallback(self):
        """Last resort: one global open-addressing table (device atomics)."""
        if self.weights is None:
            tab, st = count_into_new_table([self.keys], [self.valid], max(self.hint, 1 << 20))
        else:
            keys, weights, null_weight = self.keys, self.weights, 0
            if self.valid is not None:
                # nvt_count_merge_* takes a (key, count) list, no bitmap: the null rows leave here
                # (torch plumbing for a rare path, as unpack_bitmap) and their weights are the nulls
                ok = K.unpack_bitmap(self.valid, self.n)
                null_weight = int(weights[~ok].sum().item())
                keys, weights = keys[ok].contiguous(), weights[ok].contiguous()
            # int32 tables keep uint32 counts (include/nvt_hip.h): weighted sums may pass 2^32, so
            # int32 keys go through an int64 table, where the smallest int32 is a key like any other
            tab = CountTable(torch.int64, 2 * max(int(keys.numel()), 1))   # (rows left after the nulls)
            if keys.numel():
                tab.merge(keys.to(torch.int64), weights)
            st = tab.read_state()
            st[_lib.ST_NULLS] += null_weight
        k, c = tab.compact()
        k = k.to(self.keys.dtype)   # (the int64 table of int32 keys: every key came from an int32, exact)
        mx = int(c.max().item()) if c.numel() else 0
        self.result = (k, c, st[_lib.ST_NULLS], _plain_info(-1, int(k.numel()), mx, self.n))


def _estimate_distinct(d: int, m: int, n: int) -> int:
    """Distinct keys expected in n rows given d distinct among the first m (uniform-draw
    model d = D (1 - exp(-m / D)), tripled for the heavy tails of real categorical data).
    Only steers the first path choice: an underestimate costs one cheap failed attempt."""
    if m <= 0 or d <= 0:
        return 1
    r = d / m
    if r < 0.02:
        D = float(d)
    elif r > 0.999:
        D = float(n)
    else:
        lo, hi = 1e-6, 60.0  # x = m / D, (1 - exp(-x)) / x decreases from 1 to 0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if (1.0 - math.exp(-mid)) / mid > r:
                lo = mid
            else:
                hi = mid
        D = m / (0.5 * (lo + hi))
    return int(min(n, 3.0 * D + 64))


def _presample(jobs):
    """Jobs with no cardinality hint (first partition of a fit) start on a path chosen from
    the distinct count of a 256 K-row prefix instead of climbing PATH_ORDER from the bottom:
    the cold fit of the 45 M-row Criteo frame drops from 74 ms to under 30 ms."""
    cand = [j for j in jobs if j.result is None and j.hint <= 0 and j.weights is None
            and j.n >= SAMPLE_MIN_ROWS]
    if not cand:
        return
    if K.PRESAMPLE_SKETCH:
        # ONE launch: a HyperLogLog sketch of every column's prefix (nvt_prefix_distinct); the exact
        # count below went through ~11 launches per column for numbers that are tripled anyway
        descs = (_lib.PrefixCol * len(cand))()
        for d, j in zip(descs, cand):
            d.keys, d.valid = j.keys.data_ptr(), K.ptr(j.valid)
            d.n, d.key_bytes = min(SAMPLE_ROWS, j.n), j.kb
        out = torch.empty((len(cand), 2), dtype=torch.int64, device=cand[0].dev)
        check(cand[0].lib.nvt_prefix_distinct(descs, len(cand), out.data_ptr(), K.stream_ptr()),
              "nvt_prefix_distinct")
        res = [(None, None, 0, dict(distinct=int(d), rows=int(r))) for d, r in K.read_back(out).tolist()]
    else:
        samples = []
        for j in cand:
            valid = None if j.valid is None else j.valid[: SAMPLE_ROWS // 8]
            sj = DenseCountJob(j.keys[:SAMPLE_ROWS], valid, None, hint=SAMPLE_ROWS)
            sj.path, sj.cap_guess = 1, SAMPLE_ROWS
            samples.append(sj)
        res = CountBatch(samples, presample=False).results()
    for j, (_, _, nulls, info) in zip(cand, res):
        est = _estimate_distinct(info["distinct"], info["rows"] - nulls, j.n)
        j.hint = est
        K.stat_add("presampled_columns")
        # an estimate, not a hint: the range path starts with all its buckets (a column with more
        # keys than estimated would overflow 256 / 512 buckets and be counted twice) -- unless the
        # prefix shows every key >= 10 times on average: the estimate (3 x the uniform model) then
        # sizes the buckets.  (Heavy tails defeat any extrapolation from 0.6 % of the rows: a
        # Criteo column with 6.2 M keys shows 98 k in the prefix and is estimated at 322 k, Chao1
        # says 550 k; such columns show most prefix keys once or twice and keep 1024 buckets.)
        seen_rows = max(int(info["rows"]) - int(nulls), 1)
        j.min_range_bits = max(j.min_range_bits, 10 if int(info["distinct"]) * 10 >= seen_rows else 8)
        j.path = _path_for(est, small_tables=(j.kb == 8), allow_range=j.allow_range)
        # ... and a roomy output list (a sixth of the rows): a relaunch costs a full recount
        j.cap_guess = max(1 << 16, 2 * est, j.n // 6 if j.path not in _S_CLASSES else 0)


class CountBatch:
    """Every column's groupby-size of one partition, enqueued by ONE C call
    (nvt_dense_count_many); ``results()`` performs the single device->host read of all the
    state words and relaunches the (rare, once hints are learned) columns whose LDS tables or
    output lists overflowed.  Launch and read-back are separate so that the caller can queue
    other work (Normalize's moments, the next partition's copies) before synchronising."""

    def __init__(self, jobs, presample: bool = True):
        self.jobs = list(jobs)
        self._results = None
        if presample:
            _presample(self.jobs)
        for j in self.jobs:
            if j.n == 0:
                j.result = _empty_result(j.keys)
        for j in self.jobs:
            if j.result is None and j.path < 0:
                j._fallback()
        self.pending = [j for j in self.jobs if j.result is None]
        self.states = None
        self._launch()

    def _launch(self):
        if not self.pending:
            return
        order, slots = assign_streams([j.path for j in self.pending], [j.n for j in self.pending],
                                      K.COUNT_STREAMS, K.HEAD_START)
        pending = self.pending = [self.pending[i] for i in order]
        dev = pending[0].dev
        self.states = torch.empty(len(pending), _lib.STATE_WORDS, dtype=torch.int64, device=dev)
        descs = (_lib.CountCol * len(pending))()
        need = 0
        for i, j in enumerate(pending):
            j.state = self.states[i]
            need = max(need, j.prepare(descs[i]))
        wps = {k: _workspace(need, dev, k).data_ptr() for k in set(slots)}
        for d, k in zip(descs, slots):
            d.ws = wps[k]
        check(_lib.load().nvt_dense_count_many(descs, len(pending), K.stream_ptr()),
              "nvt_dense_count_many")
        # what results() waits for: THIS call's kernels, not whatever is queued behind them (the
        # next partition's counting is launched before this one is read back)
        self._done = torch.cuda.Event()
        self._done.record()

    def _read_states(self):
        dev = self.states.device
        side = K._check_streams.get(dev.index)
        if side is None:
            side = K._check_streams[dev.index] = torch.cuda.Stream(device=dev)
        side.wait_event(self._done)
        with torch.cuda.stream(side):
            return K.read_back(self.states).tolist()

    def results(self):
        if self._results is None:
            while self.pending:
                host = self._read_states()  # the single synchronisation point
                self.pending = [j for i, j in enumerate(self.pending) if not j.resolve(host[i])]
                K.stat_add("count_relaunches", len(self.pending))
                self._launch()
            self._results = [j.result for j in self.jobs]
        return self._results


def dense_count_many(jobs):
    """Launch every job (one C call), then ONE readback for all their state words."""
    return CountBatch(jobs).results()


def dense_count(
    keys: torch.Tensor,
    valid: Optional[torch.Tensor],
    weights: Optional[torch.Tensor] = None,
    hint: int = 0,
):
    """Groupby-size (or weighted sum) of a key column -> (keys, counts[int64], nulls, info).

    ``hint`` = expected number of distinct keys (0 = unknown).  Picks the LDS /
    partitioned path from it and escalates when a kernel reports that its LDS
    tables filled up; the last resort is the global-table kernel of nvt_count_*.
    info = dict(path, distinct, max_count, rows) so callers can remember the hint."""
    return dense_count_many([DenseCountJob(keys, valid, weights, hint)])[0]


def merge_dense(lists, hint: int = 0):
    """Tree-merge step (_mid_level_groupby): sum the counts of equal keys across
    several dense (keys, counts) lists."""
    lists = [(t[0], t[1]) + tuple(t[2:]) for t in lists if t[0].numel()]
    if not lists:
        return None
    if len(lists) == 1:
        return lists[0] if len(lists[0]) == 3 else (lists[0][0], lists[0][1], 0)
    lists = [(t[0], t[1]) for t in lists]
    dt = torch.int64 if any(k.dtype == torch.int64 for k, _ in lists) else torch.int32
    keys = torch.cat([k.to(dt) for k, _ in lists])
    counts = torch.cat([c for _, c in lists])
    k, c, _, info = dense_count(keys, None, counts,
                                hint=hint or max(int(x[0].numel()) for x in lists))
    return k, c, info["max_count"]


def merge_dense_many(groups, hints=None):
    """merge_dense for several groups with ONE nvt_dense_count_many call (and one read-back):
    groups[j] = the (keys, counts[, max_count]) lists of group j -> [(keys, counts, max_count)]."""
    jobs, slots, out = [], [], [None] * len(groups)
    for j, lists in enumerate(groups):
        lists = [(t[0], t[1]) for t in lists if t[0].numel()]
        if not lists:
            continue
        if len(lists) == 1:
            out[j] = (lists[0][0], lists[0][1], int(groups[j][0][2]) if len(groups[j][0]) > 2 else 0)
            continue
        dt = torch.int64 if any(k.dtype == torch.int64 for k, _ in lists) else torch.int32
        keys = torch.cat([k.to(dt) for k, _ in lists])
        counts = torch.cat([c for _, c in lists])
        hint = (hints[j] if hints else 0) or max(int(x[0].numel()) for x in lists)
        jobs.append(DenseCountJob(keys, None, counts, hint))
        slots.append(j)
    if jobs:
        for j, (k, c, _, info) in zip(slots, dense_count_many(jobs)):
            out[j] = (k, c, info["max_count"])
    return out


# --------------------------------------------------------------------------
# what the columns of an operator taught the driver
# --------------------------------------------------------------------------
class CountMemory:
    """Per column key: the cardinality hint and the range-path record that the next partition's
    (or fit's) DenseCountJob starts from."""

    def __init__(self):
        self.cap_hints = {}          # expected distinct keys (also: group-level merge hints)
        self.last_paths = {}         # counting path of each column's last partition
        self.no_range = set()        # columns on which the range path overflowed
        self.range_failures = []     # (column, NVT_OVF_* bits, distinct) of each overflow
        self.range_oks = {}          # partitions each column counted on the range path
        self.range_pieces = {}       # column -> int32[65] splitters (NVT_PATH_PIECES)
        self.range_bits_floor = {}   # column -> log2 buckets that held it after an overflow

    def job_args(self, hkey) -> dict:
        """The DenseCountJob arguments of a column."""
        return dict(hint=self.cap_hints.get(hkey, 0), allow_range=hkey not in self.no_range,
                    pieces=self.range_pieces.get(hkey),
                    min_range_bits=self.range_bits_floor.get(hkey, 8))

    def learn(self, hkey, dk, dc, nulls, info):
        """Digest one result (keys, counts, nulls, info) of the column."""
        old_hint = self.cap_hints.get(hkey, 0)
        self.cap_hints[hkey] = max(64, info["distinct"])
        self.last_paths[hkey] = info["path"]
        if (info.get("range_bits_floor", 8) > self.range_bits_floor.get(hkey, 8)
                and old_hint > 0 and info["distinct"] <= old_hint + old_hint // 4):
            # the buckets a GOOD hint asked for overflowed (keys not spread evenly): the next
            # partitions / fits of this column start with the bucket count that held it.  (A
            # launch without a hint, or with one the column outgrew, escalates for itself only.)
            self.range_bits_floor[hkey] = info["range_bits_floor"]
        if info.get("range_failed"):
            # one overflow does not condemn a column: the hot-key sample is a heuristic (a
            # frequent key that loses the race for its image bucket floods one region of the
            # partition pass -- about one 45 M-row partition in a hundred on the Criteo-shaped
            # columns).  Keys that are NOT spread over their range fail every time: banned
            # after two overflows making up more than a fifth of the attempts.
            self.range_failures.append((hkey, info.get("range_fail_bits", 0), info["distinct"]))
            fails = sum(1 for h, _, _ in self.range_failures if h == hkey)
            if fails >= 2 and 4 * fails > self.range_oks.get(hkey, 0):
                self.no_range.add(hkey)
        elif info["path"] == PATH_RANGE:
            self.range_oks[hkey] = self.range_oks.get(hkey, 0) + 1
        if info.get("range_failed") and info.get("sorted_by_key") and dk.dtype == torch.int32:
            # the linear range map overflowed (keys not spread over their range: dense /
            # frequency-ordered ids) and the sort path delivered the exact key-ordered list:
            # splitters of a piecewise map from it; the column's next partitions / fits take
            # the range path with them, and the overflow is not held against the column
            sp = None if info.get("range_pieces") else K.range_splitters(dk, dc)
            if info.get("range_pieces"):
                self.range_pieces.pop(hkey, None)   # overflowed WITH splitters: counts as a failure
            if sp is not None:
                self.range_pieces[hkey] = sp
                self.no_range.discard(hkey)
                self.range_failures = [f for f in self.range_failures if f[0] != hkey]
