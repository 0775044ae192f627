"""Thin, typed wrappers over the C ABI: torch tensors in, torch tensors out.

torch is used here only as the device allocator / stream provider ("plumbing");
every O(rows) computation below is a hand-written gfx950 kernel reached through
``libnvt_hip.so``.  Nothing in this module has a CPU code path.

This file is the facade of the host driver: the subjects with a module of their own
(``kernels_count.py``: Categorify's counting driver and its path policy; ``kernels_encode.py``: its
encode tables and their kind policy; ``kernels_groupby.py``, ``kernels_lookup.py``,
``kernels_exchange.py``) are re-exported at the bottom, and the switches
that tests, bench.py or a tool assign live here -- those modules read them as ``K.<NAME>`` when
they are called.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import List, Optional

import torch

from . import _lib
from ._lib import check

INT32_MIN = -(2**31)
INT64_MIN = -(2**63)

_DTYPE_CODE = {
    torch.float32: _lib.NVT_F32,
    torch.float64: _lib.NVT_F64,
    torch.int32: _lib.NVT_I32,
    torch.int64: _lib.NVT_I64,
    torch.uint8: _lib.NVT_U8,
    torch.bool: _lib.NVT_U8,
}


# --------------------------------------------------------------------------
# per-kernel timing (bench.py): HIP events recorded INSIDE the library, on the stream each
# kernel family is launched on (nvt_prof_begin / nvt_prof_report); nothing is recorded -- and
# nothing is paid -- while profiling is off
# --------------------------------------------------------------------------
def profile_begin():
    check(_lib.load().nvt_prof_begin(), "nvt_prof_begin")


def profile_report():
    """dict(kernels={name: (total_ms, launches, algorithmic_bytes)}, busy_ms, span_ms) for the
    profiled region; busy_ms = union of the recorded kernel intervals (GPU-busy time)."""
    import json

    lib = _lib.load()
    need = C.c_uint64()
    buf = C.create_string_buffer(1 << 16)
    check(lib.nvt_prof_report(buf, len(buf), C.byref(need)), "nvt_prof_report")
    rep = json.loads(buf.value.decode())
    rep["kernels"] = {k: tuple(v) for k, v in rep["kernels"].items()}
    return rep


def profile_end():
    """{kernel: (total_ms, launches, algorithmic_bytes)} for the profiled region."""
    return profile_report()["kernels"]


class annotate:
    """roctx range named after the reference's @annotate of the step being replaced
    (categorify.py:345,477,955,1054,1073,1149): attributes rocprofv3 traces to operators."""

    def __init__(self, name: str):
        self.name = name.encode()

    def __enter__(self):
        try:
            _lib.load().nvt_range_push(self.name)
            self._on = True
        except Exception:
            self._on = False
        return self

    def __exit__(self, *exc):
        if self._on:
            _lib.load().nvt_range_pop()
        return False


_event_pool = []  # handles of released Events: a fit re-uses them instead of creating new ones


class Event:
    """Opaque nvt_event (a HIP event without timing): recorded by the library behind the last
    kernel that produces an object on one of its internal streams, waited for -- on the stream,
    never on the host -- by whoever consumes the object next.  Handles are pooled: a steady-state
    fit creates and destroys no HIP objects."""

    def __init__(self):
        if _event_pool:
            self.handle = _event_pool.pop()
            return
        h = C.c_void_p()
        check(_lib.load().nvt_event_create(C.byref(h)), "nvt_event_create")
        self.handle = h

    def wait(self, stream: Optional[int] = None):
        check(_lib.load().nvt_stream_wait_event(stream_ptr() if stream is None else stream,
                                                self.handle), "nvt_stream_wait_event")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.handle = None
            try:
                if len(_event_pool) < 256:
                    _event_pool.append(h)  # waits already enqueued captured the event's state
                else:
                    _lib.load().nvt_event_destroy(h)
            except Exception:
                pass


_mailboxes = {}
READBACK_TIMEOUT_S = float(os.environ.get("NVT_READBACK_TIMEOUT", "120"))


READBACK_MEMCPY = os.environ.get("NVT_READBACK", "mailbox") == "memcpy"   # (read once, at import)


def read_back(t: torch.Tensor):
    """Small device tensor (int64 / float64) -> numpy array on the host WITHOUT a blocking
    runtime wait: one tiny kernel copies it into coherent pinned memory and the host spins on
    a sequence word (nvt_mailbox_*; include/nvt_hip.h explains why).  Stream-ordered behind
    everything queued on the current stream, like ``t.cpu()``."""
    import numpy as np

    assert t.is_cuda and t.element_size() == 8
    if READBACK_MEMCPY:
        return t.cpu().numpy()
    lib = _lib.load()
    t = t.contiguous()
    nbytes = t.numel() * 8
    key = (t.device.index, stream_ptr())
    mb = _mailboxes.get(key)
    if mb is None or lib.nvt_mailbox_capacity(mb) < nbytes:
        if mb is not None:
            lib.nvt_mailbox_destroy(mb)
        h = C.c_void_p()
        check(lib.nvt_mailbox_create(max(1 << 16, 2 * nbytes), C.byref(h)), "nvt_mailbox_create")
        mb = _mailboxes[key] = h
    if nbytes == 0:
        return np.empty(t.shape, dtype=np.int64 if t.dtype == torch.int64 else np.float64)
    seq = C.c_uint64()
    check(lib.nvt_mailbox_post(mb, t.data_ptr(), nbytes, stream_ptr(), C.byref(seq)),
          "nvt_mailbox_post")
    check(lib.nvt_mailbox_wait(mb, seq.value, READBACK_TIMEOUT_S), "nvt_mailbox_wait")
    np_dt = {torch.int64: np.int64, torch.float64: np.float64}[t.dtype]
    buf = (C.c_char * nbytes).from_address(lib.nvt_mailbox_data(mb))
    return np.frombuffer(buf, dtype=np_dt).reshape(tuple(t.shape)).copy()


class PendingReadBack:
    """read_back in two halves: the copy is enqueued by the constructor, ``get()`` waits for it.
    Between the two the host can keep enqueueing work BEHIND the copy: by the time it asks, the
    value has arrived and the device is still busy (a blocking read-back leaves the device idle
    for as long as the host needs to reach its next launch)."""

    _free = {}   # (device, stream) -> idle mailboxes of this kind (each holds one value at a time)

    def __init__(self, t: torch.Tensor):
        import numpy as np

        assert t.is_cuda and t.element_size() == 8
        self._np = np
        self.shape, self.dtype = tuple(t.shape), t.dtype
        self.nbytes = t.numel() * 8
        self.value = self.mb = None
        if READBACK_MEMCPY or self.nbytes == 0:
            self.value = (t.cpu().numpy() if self.nbytes else
                          np.empty(self.shape, dtype=np.int64 if t.dtype == torch.int64 else np.float64))
            return
        lib = _lib.load()
        t = t.contiguous()
        self.key = (t.device.index, stream_ptr())
        with LAUNCH_LOCK:
            pool = self._free.setdefault(self.key, [])
            mb = None
            for i, cand in enumerate(pool):
                if lib.nvt_mailbox_capacity(cand) >= self.nbytes:
                    mb = pool.pop(i)
                    break
        if mb is None:
            h = C.c_void_p()
            check(lib.nvt_mailbox_create(max(1 << 12, self.nbytes), C.byref(h)), "nvt_mailbox_create")
            mb = h
        self.mb = mb
        seq = C.c_uint64()
        check(lib.nvt_mailbox_post(mb, t.data_ptr(), self.nbytes, stream_ptr(), C.byref(seq)), "nvt_mailbox_post")
        self.seq = seq.value
        self._keep = t

    def __del__(self):
        # never asked for (a fit whose scalars nobody read): the mailbox goes back to the pool --
        # its next post is ordered behind this one on the same stream and carries a later sequence
        mb = getattr(self, "mb", None)
        if mb is not None and getattr(self, "value", None) is None:
            try:
                with LAUNCH_LOCK:
                    self._free.setdefault(self.key, []).append(mb)
            except Exception:   # (interpreter shutdown)
                pass

    def get(self):
        if self.value is None:
            lib = _lib.load()
            check(lib.nvt_mailbox_wait(self.mb, self.seq, READBACK_TIMEOUT_S), "nvt_mailbox_wait")
            np_dt = {torch.int64: self._np.int64, torch.float64: self._np.float64}[self.dtype]
            buf = (C.c_char * self.nbytes).from_address(lib.nvt_mailbox_data(self.mb))
            self.value = self._np.frombuffer(buf, dtype=np_dt).reshape(self.shape).copy()
            with LAUNCH_LOCK:
                self._free.setdefault(self.key, []).append(self.mb)
            self.mb = self._keep = None
        return self.value


def read_back_ptr(ptr: int, nwords: int, device_index: int):
    """uint64[nwords] at device address ``ptr`` -> list of ints, through the mailbox."""
    import numpy as np

    lib = _lib.load()
    nbytes = nwords * 8
    key = (device_index, stream_ptr())
    mb = _mailboxes.get(key)
    if mb is None or lib.nvt_mailbox_capacity(mb) < nbytes:
        if mb is not None:
            lib.nvt_mailbox_destroy(mb)
        h = C.c_void_p()
        check(lib.nvt_mailbox_create(max(1 << 16, 2 * nbytes), C.byref(h)), "nvt_mailbox_create")
        mb = _mailboxes[key] = h
    seq = C.c_uint64()
    check(lib.nvt_mailbox_post(mb, ptr, nbytes, stream_ptr(), C.byref(seq)), "nvt_mailbox_post")
    check(lib.nvt_mailbox_wait(mb, seq.value, READBACK_TIMEOUT_S), "nvt_mailbox_wait")
    buf = (C.c_char * nbytes).from_address(lib.nvt_mailbox_data(mb))
    return np.frombuffer(buf, dtype=np.uint64).astype(np.int64).tolist()


class _timed:
    """Former Python-side event bracket; timing now lives in the library (NVT_PROF scopes)."""

    def __init__(self, name, alg_bytes):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DTYPE_CODE[dt]
    except KeyError:
        raise TypeError(f"unsupported column dtype {dt}") from None


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def aligned(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Contiguous and 16-byte aligned (views with a storage offset get copied)."""
    if t is None:
        return None
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def next_pow2(x: int) -> int:
    return 1 << max(6, (int(x) - 1).bit_length())


def _key_suffix(keys: torch.Tensor) -> str:
    if keys.dtype == torch.int32:
        return "i32"
    if keys.dtype == torch.int64:
        return "i64"
    raise TypeError(f"categorical keys must be int32/int64 on device, got {keys.dtype}")


# --------------------------------------------------------------------------
# Categorify.fit counting (kernels_count.py): what tests, bench.py and tools set on the facade
# --------------------------------------------------------------------------
PATH_TINY_MAX = 64                  # path 6: path 0 with hot keys replicated per lane group
# most distinct keys the range path (path 9) is started on; beyond: the sort path
PATH_RANGE_MAX_DISTINCT = int(os.environ.get("NVT_RANGE_MAX", 6_500_000))
RANGE_PIECES = 64   # nvt_range.hpp kRpPieces: pieces of the piecewise range map (range_splitters)
_check_streams = {}   # device index -> side stream of the read-backs that must not wait for work queued later
# Columns of one nvt_dense_count_many call that are given different workspaces run on different
# internal streams (include/nvt_hip.h); COUNT_STREAMS workspaces are kept per device.
COUNT_STREAMS = max(1, min(3, int(os.environ.get("NVT_COUNT_STREAMS", "3"))))
# columns that need no hot-key sample start the counting streams (they run under the sample launch)
HEAD_START = os.environ.get("NVT_COUNT_HEAD_START", "1") != "0"
STATS = {"count_relaunches": 0, "presampled_columns": 0}  # diagnostics (bench.py cold step)
PRESAMPLE_SKETCH = os.environ.get("NVT_PRESAMPLE_EXACT", "0") != "1"


MERGE_SORTED_MAX_TOTAL = (1 << 31) - 1   # include/nvt_hip.h nvt_merge_sorted_many: na + nb < 2^31


def merge_sorted_pairs(pairs, want_src: bool = False):
    """nvt_merge_sorted_many: pairs = [((keys_a, counts_a), (keys_b, counts_b))] of KEY-SORTED,
    duplicate-free int32 lists (counts int64 or None) -> [(keys, counts)] -- the union in key
    order, counts of equal keys summed; with want_src [(keys, counts, src_a, src_b)] where
    src_* = the position in A / B an output entry came from (-1: none).  ONE merge-path launch +
    ONE tile launch for all pairs, ONE read-back (the merged lengths)."""
    if not pairs:
        return []
    _lib.require_gpu()
    lib = _lib.load()
    dev = pairs[0][0][0].device
    descs = (_lib.MergeCol * len(pairs))()
    out_n = torch.empty(len(pairs), dtype=torch.int64, device=dev)
    outs, keep = [], []
    # ONE output buffer per array for the whole call (a multi-GPU owner merges ~100 pairs per
    # level: four allocations per pair were most of the call), every pair on a 16-byte boundary
    sizes, offs, tot = [], [], 0
    for (ka, _), (kb, _) in pairs:
        n_ab = int(ka.numel()) + int(kb.numel())
        if n_ab > MERGE_SORTED_MAX_TOTAL:
            raise _lib.NvtHipError("merge_sorted_pairs: more than 2^31 - 1 entries in one merge")
        sizes.append(n_ab)
        offs.append(tot)
        tot += (max(n_ab, 1) + 3) // 4 * 4   # (at least one element: an empty pair must still look
                                            # like "with src maps" to the library)
    with_counts = any(ca is not None or cb is not None for (_, ca), (_, cb) in pairs)
    ok_all = torch.empty(tot, dtype=torch.int32, device=dev)
    oc_all = torch.empty(tot, dtype=torch.int64, device=dev) if with_counts else None
    sa_all = torch.empty(tot, dtype=torch.int32, device=dev) if want_src else None
    sb_all = torch.empty(tot, dtype=torch.int32, device=dev) if want_src else None
    pk, pc = ok_all.data_ptr(), oc_all.data_ptr() if oc_all is not None else 0
    psa, psb = (sa_all.data_ptr(), sb_all.data_ptr()) if want_src else (0, 0)
    pn = out_n.data_ptr()
    for i, (d, ((ka, ca), (kb, cb))) in enumerate(zip(descs, pairs)):
        assert ka.dtype == torch.int32 and kb.dtype == torch.int32
        ka, kb = ka.contiguous(), kb.contiguous()
        ca = ca.contiguous() if ca is not None else None
        cb = cb.contiguous() if cb is not None else None
        na, nb = int(ka.numel()), int(kb.numel())
        has_c = ca is not None or cb is not None
        o = offs[i]
        d.a_keys, d.a_counts, d.na = ptr(ka) if na else None, ptr(ca) if na else None, na
        d.b_keys, d.b_counts, d.nb = ptr(kb) if nb else None, ptr(cb) if nb else None, nb
        d.out_keys, d.out_counts = pk + 4 * o, (pc + 8 * o) if has_c else None
        d.src_a, d.src_b = (psa + 4 * o, psb + 4 * o) if want_src else (None, None)
        d.out_n = pn + 8 * i
        outs.append((o, has_c))
        keep.append((ka, kb, ca, cb))
    need = C.c_uint64()
    check(lib.nvt_merge_sorted_ws_bytes(descs, len(pairs), C.byref(need)), "nvt_merge_sorted_ws_bytes")
    ws = torch.empty(need.value + 16, dtype=torch.uint8, device=dev)
    check(lib.nvt_merge_sorted_many(descs, len(pairs), ws.data_ptr(), need.value, stream_ptr()),
          "nvt_merge_sorted_many")
    ns = read_back(out_n).tolist()
    res = []
    for (o, has_c), n in zip(outs, ns):
        n = int(n)
        if want_src:
            res.append((ok_all[o:o + n], oc_all[o:o + n] if has_c else None, sa_all[o:o + n], sb_all[o:o + n]))
        else:
            res.append((ok_all[o:o + n], oc_all[o:o + n] if has_c else None))
    return res


def merge_payload(src_a, src_b, a, b, op: str = "add", width: int = 1):
    """nvt_merge_payload: rows of ``width`` int64 / float64 values of two merged lists combined
    through the src maps of merge_sorted_pairs (op: add / min / max; a missing side contributes
    nothing).  a, b: [entries * width] contiguous."""
    n = int(src_a.numel())
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.dtype in (torch.int64, torch.float64)
    out = torch.empty(n * width, dtype=a.dtype, device=src_a.device)
    check(_lib.load().nvt_merge_payload(
        ptr(src_a), ptr(src_b), n, int(width), dtype_code(a.dtype), {"add": 0, "min": 1, "max": 2}[op],
        ptr(a) if a.numel() else None, ptr(b) if b.numel() else None, out.data_ptr(), stream_ptr()),
        "nvt_merge_payload")
    return out


def merge_sorted_tree(col_lists):
    """Tree merge (_mid_level_groupby, categorify.py:1054-1070, over the tree of :1423-1478) of
    KEY-SORTED (keys int32, counts int64) lists: col_lists[j] = the lists of column j; returns
    one (keys, counts) per column.  Every level merges disjoint pairs of ALL columns in one
    call (nvt_merge_sorted_many) and costs one read-back; a list much larger than the others
    (the table accumulated so far) is held back for the last level, so it is streamed once."""
    cur = [[(k, c) for k, c in lists if int(k.numel())] for lists in col_lists]
    while any(len(l) > 1 for l in cur):
        pairs, plan = [], []
        for j, lists in enumerate(cur):
            if len(lists) < 2:
                plan.append((j, [], lists))
                continue
            order = sorted(lists, key=lambda t: int(t[0].numel()))
            held = []
            if len(order) > 2 and int(order[-1][0].numel()) > 2 * int(order[-2][0].numel()):
                held = [order.pop()]
            mine = []
            while len(order) >= 2:
                a, b = order.pop(0), order.pop(0)
                mine.append(len(pairs))
                pairs.append((a, b))
            plan.append((j, mine, order + held))
        merged = merge_sorted_pairs(pairs)
        cur = [[merged[i] for i in mine] + rest for j, mine, rest in plan]
    devs = [t[0].device for lists in col_lists for t in lists]
    dev = devs[0] if devs else torch.device("cuda", torch.cuda.current_device())
    out = []
    for lists in cur:
        out.append(lists[0] if lists else (torch.empty(0, dtype=torch.int32, device=dev),
                                           torch.empty(0, dtype=torch.int64, device=dev)))
    return out


def range_splitters(keys: torch.Tensor, counts: torch.Tensor, rows: int = 0):
    """int32[65] splitters of the piecewise range map (NVT_PATH_PIECES) from an EXACT key-ordered
    (key, count) list of the column (what the sort path returns after the linear map
    overflowed), or None when the list is too short to need them.

    The range path wants buckets with at most ~2x the average of (a) the rows that go through
    the partition bins and (b) the distinct keys of a bucket table.  Every key gets the weight
    1/3 x its share of the bin rows (the ~8192 most frequent keys, which the hot image mostly
    absorbs, count with a third of their rows) + 2/3 x its share of the distinct keys (1 / entries); splitter p
    is the key at which the running weight reaches p / 64.  Values are the order-preserving
    uint32 images of the keys (key ^ 2^31), stored in an int32 tensor.  One read-back."""
    n = int(keys.numel())
    if n < 4096 or keys.dtype != torch.int32:
        return None
    k64 = keys.to(torch.int64)
    if int(k64[0].item()) == INT32_MIN:   # the sentinel key leads the list and is not in any table
        k64, counts, n = k64[1:], counts[1:], n - 1
    c = counts.to(torch.float64)
    rows = rows or float(c.sum().item())
    # rows that go through the bins = rows of the keys that are NOT in the hot image.  The image
    # (hot_sample_kernel) takes the keys the 64 K-row sample shows twice, the most frequent ones
    # first; a key with lam expected sample hits is in with about P(Poisson(lam) >= 2), less the
    # bucket conflicts of the late-comers (2-slot buckets: ~15 %); lam >= 8: practically always
    lam = c * (65536.0 / max(float(rows), 1.0))
    p_in = torch.where(lam >= 8.0, torch.full_like(c, 0.98),
                       0.85 * (1.0 - torch.exp(-lam) * (1.0 + lam)))
    w_rows = c * (1.0 - p_in)
    tot = w_rows.sum()
    w = (2.0 / 3.0) / n + torch.where(tot > 0, w_rows / torch.clamp(tot, min=1.0) / 3.0, torch.zeros_like(c) + (1.0 / 3.0) / n)
    cum = torch.cumsum(w, 0)
    cum = cum / cum[-1]
    targets = torch.arange(1, RANGE_PIECES, dtype=torch.float64, device=keys.device) / RANGE_PIECES
    idx = torch.searchsorted(cum, targets).clamp_(max=n - 1)
    u = (torch.cat([k64[:1], k64[idx], k64[-1:] + 1]) + (1 << 31))
    host = read_back(u).tolist()
    for p in range(1, RANGE_PIECES + 1):      # strictly increasing (degenerate pieces: one key wide)
        if host[p] <= host[p - 1]:
            host[p] = host[p - 1] + 1
    if host[-1] > 0xFFFFFFFF:
        return None
    arr = torch.tensor(host, dtype=torch.int64, device=keys.device)
    return torch.where(arr >= (1 << 31), arr - (1 << 32), arr).to(torch.int32)   # the u32 bit pattern


def class_hist(counts: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32[256] histogram of min(count, 255) on the device (nvt_class_hist): the input of the
    one-pass ordering of a key-sorted (key, count) list.  out: a contiguous int32[256] to fill."""
    hist = out if out is not None else torch.empty(256, dtype=torch.int32, device=counts.device)
    counts = counts.contiguous()
    check(_lib.load().nvt_class_hist(ptr(counts) if counts.numel() else None, counts.numel(),
                                     hist.data_ptr(), stream_ptr()), "nvt_class_hist")
    return hist


def label_shard(keys: torch.Tensor, counts: torch.Tensor, class_base_diff: torch.Tensor, n_big: int,
                label_of: torch.Tensor):
    """nvt_vocab_label_shard: positions in the vocabulary order of the UNION for this rank's shard
    of a key-sorted (key, count) list (entries with count < 255; the others -1), written into
    ``label_of`` (int32[n]); returns (big_keys, big_counts, big_src) of the n_big entries with
    count >= 255, compacted in key order (big_src: their positions in the shard)."""
    n = int(keys.numel())
    dev = keys.device
    bk = torch.empty(max(n_big, 1), dtype=torch.int32, device=dev)
    bc = torch.empty(max(n_big, 1), dtype=torch.int64, device=dev)
    bs = torch.empty(max(n_big, 1), dtype=torch.int32, device=dev)
    if n == 0:
        return bk[:0], bc[:0], bs[:0]
    lib = _lib.load()
    out = C.c_uint64()
    check(lib.nvt_vocab_order_tmp_bytes(n, 0, C.byref(out)), "nvt_vocab_order_tmp_bytes")
    tmp = torch.empty(out.value + 16, dtype=torch.uint8, device=dev)
    check(lib.nvt_vocab_label_shard(keys.contiguous().data_ptr(), counts.contiguous().data_ptr(), n,
                                    class_base_diff.data_ptr(), tmp.data_ptr(), label_of.data_ptr(),
                                    bk.data_ptr(), bc.data_ptr(), bs.data_ptr(), stream_ptr()),
          "nvt_vocab_label_shard")
    return bk[:n_big], bc[:n_big], bs[:n_big]


def sort_by_key(keys: torch.Tensor, counts: torch.Tensor):
    """(keys, counts) ordered by key ascending (radix sort of nvt_order_rows)."""
    n = int(keys.numel())
    if n <= 1:
        return keys, counts
    perm = order_rows(n, keys.device, sort_keys=[(keys, None, True)]) & 0xFFFFFFFF
    return keys[perm].contiguous(), counts[perm].contiguous()


def vocab_sort(keys: torch.Tensor, counts: torch.Tensor, max_count: int = 0):
    """In place: (count desc, key asc) -- categorify.py:1300,1316 with the stable tie rule.
    max_count (upper bound on counts, 0 = unknown) avoids a stream synchronisation."""
    lib = _lib.load()
    n = keys.numel()
    if n <= 1:
        return
    suffix = _key_suffix(keys)
    nbytes = C.c_uint64()
    check(lib.nvt_vocab_sort_tmp_bytes(4 if suffix == "i32" else 8, n, C.byref(nbytes)))
    tmp = torch.empty(nbytes.value + 16, dtype=torch.uint8, device=keys.device)
    assert keys.is_contiguous() and counts.is_contiguous()
    with _timed("vocab_sort", 0):
        check(
            getattr(lib, f"nvt_vocab_sort_{suffix}")(
                keys.data_ptr(), counts.data_ptr(), n, int(max_count), tmp.data_ptr(), stream_ptr()
            ),
            "nvt_vocab_sort",
        )


# --------------------------------------------------------------------------
# Categorify.transform (kernels_encode.py): what bench.py and A / B runs set on the facade
# --------------------------------------------------------------------------
ASYNC_FINALIZE = os.environ.get("NVT_ASYNC_FINALIZE", "1") != "0"


# --------------------------------------------------------------------------
# continuous columns
# --------------------------------------------------------------------------
_scratch = {}


def _partials(device) -> torch.Tensor:
    # one scratch block per (device, stream): reductions of different operators may be in
    # flight on different streams at the same time
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    if key not in _scratch:
        nbytes = _lib.load().nvt_moments_scratch_bytes()
        _scratch[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    return _scratch[key]


def numeric(x: torch.Tensor) -> torch.Tensor:
    """A bool / uint8 column as int64 (``nvt_widen_i64``): the continuous kernels have no 1-byte
    instantiations, so such a column is widened first, the way LogOp and Bucketize take it."""
    return widen_i64(x) if x.dtype in (torch.bool, torch.uint8) else x


def _check_int_params(what: str, dtype: torch.dtype, **params):
    """The integer-in / integer-out kernels take their constants as doubles and convert them to
    the column type: a constant must be an integer the type holds, and at most 2**53 in
    magnitude so that the double carries it exactly."""
    info = torch.iinfo(dtype)
    lo, hi = max(info.min, -(2**53)), min(info.max, 2**53)
    for name, b in params.items():
        if b is None:
            continue
        if b != b or b in (float("inf"), float("-inf")) or int(b) != b or not lo <= int(b) <= hi:
            raise ValueError(
                f"{what}: {name}={b!r} is not an integer in [{lo}, {hi}] that a {dtype} column "
                f"can take exactly; use a float64 output for it")


def moments_accumulate(
    x: torch.Tensor, valid: Optional[torch.Tensor], out3: torch.Tensor, fill: Optional[float] = None
):
    """out3 (float64[3] on device) += {count, sum, sum of squares}."""
    _lib.require_gpu()
    x = aligned(numeric(x))
    with _timed("moments", x.numel() * x.element_size()):
        check(
            _lib.load().nvt_moments(
                x.data_ptr(), dtype_code(x.dtype), ptr(valid), x.numel(),
                0 if fill is None else 1, 0.0 if fill is None else float(fill), out3.data_ptr(),
                _partials(x.device).data_ptr(), stream_ptr(),
            ),
            "nvt_moments",
        )


def moments_many(items):
    """items: [(x, valid, fill or None, out3)]: out3 (float64[3] on device) += {count, sum,
    sum of squares}; one launch for all columns (nvt_moments_many)."""
    if not items:
        return
    _lib.require_gpu()
    lib = _lib.load()
    descs = (_lib.MomentsCol * len(items))()
    keep = []
    for d, (x, valid, fill, out3) in zip(descs, items):
        x = aligned(numeric(x))
        keep.append(x)
        d.x = x.data_ptr()
        d.valid = ptr(valid)
        d.n = x.numel()
        d.dtype = dtype_code(x.dtype)
        d.has_fill = 0 if fill is None else 1
        d.fill_val = 0.0 if fill is None else float(fill)
        d.out3 = out3.data_ptr()
    dev = keep[0].device
    key = ("many", dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    per = lib.nvt_moments_scratch_bytes() // 8
    buf = _scratch.get(key)
    if buf is None or buf.numel() < per * len(items):
        buf = _scratch[key] = torch.empty(per * len(items), dtype=torch.float64, device=dev)
    check(lib.nvt_moments_many(descs, len(items), buf.data_ptr(), stream_ptr()), "nvt_moments_many")


# accumulator row of col_profile_many: int64[6] = {rows, valid rows, min, max, sum, sum of squares};
# min / max are int64 for an integer column and float64 bits for a float column, the sums float64 bits
PROFILE_WORDS = 6
_INT64_MAX, _INT64_MIN = (1 << 63) - 1, -(1 << 63)


def profile_is_float(dt: torch.dtype) -> bool:
    return dt in (torch.float32, torch.float64)


def new_profile_acc(dtypes, device) -> torch.Tensor:
    """int64 [len(dtypes), PROFILE_WORDS] on ``device``, every row empty: counts and sums 0, extrema
    INT64_MAX / INT64_MIN (integer column; bool / uint8 count as integers) or NaN (float column)."""
    import numpy as np

    host = np.zeros((len(dtypes), PROFILE_WORDS), dtype=np.int64)
    for i, dt in enumerate(dtypes):
        if profile_is_float(dt):
            host[i, 2:4] = np.array([np.nan, np.nan]).view(np.int64)
        else:
            host[i, 2:4] = (_INT64_MAX, _INT64_MIN)
    return torch.from_numpy(host).to(device)


def profile_rows(host, dtypes):
    """The rows of a profile accumulator on the host (numpy int64 [k, PROFILE_WORDS]) as Python
    scalars: [dict(rows, valid, min, max, sum, sumsq)]; min / max are exact ints for an integer
    column, floats for a float column, None when no row counted."""
    import numpy as np

    host = np.ascontiguousarray(host, dtype=np.int64).reshape(-1, PROFILE_WORDS)
    out = []
    for row, dt in zip(host, dtypes):
        valid = int(row[1])
        lo, hi = (row[2:4].view(np.float64).tolist() if profile_is_float(dt) else row[2:4].tolist())
        s, s2 = row[4:6].view(np.float64).tolist()
        out.append(dict(rows=int(row[0]), valid=valid, min=lo if valid else None,
                        max=hi if valid else None, sum=s, sumsq=s2))
    return out


def col_profile_many(items):
    """items: [(x, valid, acc_row)]: acc_row (one row of ``new_profile_acc`` made for x's dtype) takes
    rows, valid rows, min, max, sum and sum of squares of x -- every column in ONE read, one launch
    for all of them (nvt_col_profile_many).  x may be a slice: only element alignment is needed.
    A bool / uint8 column is widened to int64 first and a non-contiguous one is copied: one extra
    pass and a temporary for such a column in front of the one read."""
    if not items:
        return
    _lib.require_gpu()
    lib = _lib.load()
    descs = (_lib.ProfileCol * len(items))()
    keep = []
    for d, (x, valid, acc) in zip(descs, items):
        x = numeric(x)
        x = x if x.is_contiguous() else x.contiguous()
        assert acc.dtype == torch.int64 and acc.is_contiguous() and int(acc.numel()) == PROFILE_WORDS
        keep.append(x)
        d.x = x.data_ptr()
        d.valid = ptr(valid)
        d.n = x.numel()
        d.dtype = dtype_code(x.dtype)
        base = acc.data_ptr()
        d.counts, d.extrema, d.sums = base, base + 16, base + 32
    dev = keep[0].device
    key = ("profile", dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _scratch.get(key)
    if buf is None:
        buf = _scratch[key] = torch.empty(_lib.PROFILE_SCRATCH_BYTES // 8, dtype=torch.int64, device=dev)
    check(lib.nvt_col_profile_many(descs, len(items), buf.data_ptr(), stream_ptr()), "nvt_col_profile_many")


_CAST_CODE = {torch.int8: _lib.NVT_I8, torch.int16: _lib.NVT_I16, torch.int32: _lib.NVT_I32,
              torch.int64: _lib.NVT_I64, torch.float32: _lib.NVT_F32, torch.float64: _lib.NVT_F64}


def cast_many(items):
    """items: [(x, dst_dtype[, out])] -> [out]: int32 / int64 to a narrower integer (the low bits:
    numpy's astype) and float64 to float32, one launch for all columns (nvt_cast_many).  A cast to
    x's own dtype returns x itself: no launch, no copy.  Any other pair raises."""
    outs, jobs = [], []
    for item in items:
        x, dst = item[0], item[1]
        if x.dtype == dst:
            outs.append(x)
            continue
        if x.dtype not in _CAST_CODE or dst not in _CAST_CODE:
            raise TypeError(f"cast_many: unsupported cast {x.dtype} -> {dst}")
        x = x if x.is_contiguous() else x.contiguous()
        out = item[2] if len(item) > 2 else torch.empty(x.numel(), dtype=dst, device=x.device)
        assert out.dtype == dst and out.is_contiguous() and int(out.numel()) >= int(x.numel())
        jobs.append((x, out))
        outs.append(out)
    if jobs:
        _lib.require_gpu()
        descs = (_lib.CastCol * len(jobs))()
        for d, (x, out) in zip(descs, jobs):
            d.src, d.dst, d.n = x.data_ptr(), out.data_ptr(), x.numel()
            d.src_dtype, d.dst_dtype = _CAST_CODE[x.dtype], _CAST_CODE[out.dtype]
        check(_lib.load().nvt_cast_many(descs, len(jobs), stream_ptr()), "nvt_cast_many")
    return outs


def fill_normalize_many(items):
    """items: [(x, valid, fill, do_norm, shift, scale, out_dtype, want_filled_mask[, moments])] ->
    [(out, filled or None)]; one launch per dtype combination (nvt_fill_normalize_many).
    ``moments``: float64 {count, sum, sum of squares} of the column on the device -- shift / scale
    are then finished from them by the kernel (a fit whose moments are still on their way to the
    host)."""
    if not items:
        return []
    _lib.require_gpu()
    descs = (_lib.FillNormCol * len(items))()
    outs, keep = [], []
    for d, item in zip(descs, items):
        x, valid, fill, do_norm, shift, scale, out_dtype, want_mask = item[:8]
        moments = item[8] if len(item) > 8 else None
        x = aligned(x)
        keep.append(x)
        if not out_dtype.is_floating_point:
            _check_int_params("fill_normalize_many", out_dtype, fill=fill)
        if moments is not None:
            assert moments.dtype == torch.float64 and moments.is_contiguous() and int(moments.numel()) >= 3
            keep.append(moments)
        d.moments = ptr(moments)
        n = x.numel()
        out = torch.empty(n, dtype=out_dtype, device=x.device)
        filled = torch.empty(n, dtype=torch.uint8, device=x.device) if want_mask else None
        d.x = x.data_ptr()
        d.valid = ptr(valid)
        d.n = n
        d.dtype = dtype_code(x.dtype)
        d.has_fill = 0 if fill is None else 1
        d.fill_val = 0.0 if fill is None else float(fill)
        d.do_norm = 1 if do_norm else 0
        d.out_dtype = dtype_code(out_dtype)
        d.shift = float(shift)
        d.scale = float(scale)
        d.out = out.data_ptr()
        d.filled = ptr(filled)
        outs.append((out, filled.view(torch.bool) if filled is not None else None))
    check(_lib.load().nvt_fill_normalize_many(descs, len(items), stream_ptr()),
          "nvt_fill_normalize_many")
    return outs


def minmax_accumulate(x: torch.Tensor, valid: Optional[torch.Tensor], out2: torch.Tensor, first: bool):
    _lib.require_gpu()
    x = aligned(x)
    check(
        _lib.load().nvt_minmax(
            x.data_ptr(), dtype_code(x.dtype), ptr(valid), x.numel(), 0 if first else 1,
            out2.data_ptr(), _partials(x.device).data_ptr(), stream_ptr(),
        ),
        "nvt_minmax",
    )


def fill_normalize(
    x: torch.Tensor,
    valid: Optional[torch.Tensor],
    fill: Optional[float],
    do_norm: bool,
    shift: float,
    scale: float,
    out_dtype: torch.dtype,
    want_filled_mask: bool = False,
):
    _lib.require_gpu()
    x = aligned(x)
    n = x.numel()
    if not out_dtype.is_floating_point:
        _check_int_params("fill_normalize", out_dtype, fill=fill)
    out = torch.empty(n, dtype=out_dtype, device=x.device)
    filled = torch.empty(n, dtype=torch.uint8, device=x.device) if want_filled_mask else None
    with _timed("fill_normalize", n * (x.element_size() + out.element_size())):
        check(
            _lib.load().nvt_fill_normalize(
                x.data_ptr(), dtype_code(x.dtype), ptr(valid), n, 0 if fill is None else 1,
                0.0 if fill is None else float(fill), 1 if do_norm else 0, float(shift),
                float(scale), out.data_ptr(), dtype_code(out_dtype), ptr(filled), stream_ptr(),
            ),
            "nvt_fill_normalize",
        )
    return out, (filled.view(torch.bool) if filled is not None else None)


def clip_log(x, valid, fill, vmin, vmax, do_log: bool, out_dtype: torch.dtype) -> torch.Tensor:
    """Clip / LogOp pass (optionally consuming a pending FillMissing constant).  Integer in ->
    the same integer type out clamps in that type: values inside the bounds are untouched."""
    _lib.require_gpu()
    x = aligned(x)
    n = x.numel()
    if not out_dtype.is_floating_point:
        # a bound at or beyond the end of the type clips nothing (no value compares past it)
        info = torch.iinfo(out_dtype)
        if vmin is not None and vmin <= info.min:
            vmin = None
        if vmax is not None and vmax >= info.max:
            vmax = None
        _check_int_params("clip_log", out_dtype, fill=fill, min_value=vmin, max_value=vmax)
    out = torch.empty(n, dtype=out_dtype, device=x.device)
    with _timed("clip_log", n * (x.element_size() + out.element_size())):
        check(
            _lib.load().nvt_clip_log(
                x.data_ptr(), dtype_code(x.dtype), ptr(valid), n, 0 if fill is None else 1,
                0.0 if fill is None else float(fill), 0 if vmin is None else 1,
                0.0 if vmin is None else float(vmin), 0 if vmax is None else 1,
                0.0 if vmax is None else float(vmax), 1 if do_log else 0, out.data_ptr(),
                dtype_code(out_dtype), stream_ptr(),
            ),
            "nvt_clip_log",
        )
    return out


def bucketize(x: torch.Tensor, valid, boundaries: torch.Tensor) -> torch.Tensor:
    """np.digitize(x, boundaries, right=False) as int32; boundaries float64 ascending on device."""
    _lib.require_gpu()
    x = x.contiguous()
    out = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    check(
        _lib.load().nvt_bucketize(x.data_ptr(), dtype_code(x.dtype), ptr(valid), x.numel(),
                                  ptr(boundaries), int(boundaries.numel()), out.data_ptr(),
                                  stream_ptr()),
        "nvt_bucketize",
    )
    return out


def widen_i64(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == torch.int64:
        return x
    _lib.require_gpu()
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    x = x.contiguous()
    out = torch.empty(x.numel(), dtype=torch.int64, device=x.device)
    check(
        _lib.load().nvt_widen_i64(x.data_ptr(), dtype_code(x.dtype), x.numel(), out.data_ptr(),
                                  stream_ptr()),
        "nvt_widen_i64",
    )
    return out


def unpack_bitmap(valid: torch.Tensor, n: int) -> torch.Tensor:
    """Arrow validity bitmap -> bool[n] on the device (torch plumbing for rare paths: combo
    Categorify null rows).  Replaces a device -> host -> device round trip per column."""
    shifts = torch.arange(8, device=valid.device, dtype=torch.uint8)
    bits = (valid[: (n + 7) // 8].unsqueeze(1) >> shifts) & 1
    return bits.reshape(-1)[:n].to(torch.bool)


def expand_valid(packed: torch.Tensor, bitmap: torch.Tensor, n: int) -> torch.Tensor:
    """The non-null values ``packed`` (in order) under an Arrow validity bitmap -> one slot for each
    of the ``n`` positions (nvt_expand_valid); no values at all: zeros.  Enqueued on the current
    stream with a workspace of its own, so the parquet prefetcher's thread calls it without
    LAUNCH_LOCK, as it always has."""
    if packed.numel() == 0:
        return torch.zeros(n, dtype=packed.dtype, device=packed.device)
    lib = _lib.load()
    out = torch.empty(n, dtype=packed.dtype, device=packed.device)
    need = C.c_uint64()
    check(lib.nvt_expand_valid_ws_bytes(n, C.byref(need)), "nvt_expand_valid_ws_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=packed.device)
    check(lib.nvt_expand_valid(packed.data_ptr(), packed.element_size(), bitmap.data_ptr(), n, out.data_ptr(),
                               ws.data_ptr(), stream_ptr()), "nvt_expand_valid")
    return out


def popcount(valid: Optional[torch.Tensor], n: int) -> int:
    if valid is None:
        return n
    _lib.require_gpu()
    out = torch.zeros(1, dtype=torch.int64, device=valid.device)
    check(_lib.load().nvt_popcount(valid.data_ptr(), n, out.data_ptr(), stream_ptr()), "nvt_popcount")
    return int(out.item())


# ---- one int32 key column: groupby-aggregate by sorting + flat index -------------------------
SORTED_GROUPBY = os.environ.get("NVT_SORTED_GROUPBY", "1") != "0"
SORTED_GROUPBY_MIN_ROWS = 1 << 15   # below: launch latency, the hash update is as good
SORTED_GROUPBY_MAX_KFOLD = 16
FLAT_INDEX_LOAD = float(os.environ.get("NVT_FLAT_INDEX_LOAD", "0.5"))


# sorted words shared between the aggregates of ONE pass over one partition (Workflow.fit opens
# and closes it around the partition's fit_partition calls; None = no sharing).  Per THREAD: dask
# worker threads of the reference call transform concurrently on different partitions of one
# fitted workflow (SURVEY 8(b) "Threading", categorify.py:1632,1813) -- a pass and what it shares
# belong to the thread that walks the partition.
_TLS = threading.local()


def current_pass_memo():
    """The memo of the pass this THREAD is inside of, or None."""
    return getattr(_TLS, "memo", None)


class pass_memo:
    """``with K.pass_memo():`` -- results that depend only on a partition's columns (the sorted
    (key, row) words of the sort-path groupby) are shared between the operators fitted inside."""

    def __enter__(self):
        self.prev = current_pass_memo()
        _TLS.memo = {}
        return self

    def __exit__(self, *exc):
        _TLS.memo = self.prev
        return False


# Host-side launch sequences (workspaces and scratch buffers cached per (device, stream), the
# read-back mailboxes, the operators' lazily finalised vocabularies and lookup images) are
# serialised by ONE re-entrant lock taken around every operator call (ops/base.py wraps
# transform / fit_partition / fit_end / fit_finalize of every Operator subclass): threads
# interleave at operator granularity, the GPU work stays asynchronous on its streams.
LAUNCH_LOCK = threading.RLock()


def stat_add(name: str, k: int = 1):
    with LAUNCH_LOCK:
        STATS[name] = STATS.get(name, 0) + k


SHARE_SORTED_VALUES = os.environ.get("NVT_SHARE_SORTED_VALUES", "1") != "0"


EXCHANGE_MAX_COLS, EXCHANGE_MAX_CELLS = 64, 4096   # include/nvt_hip.h nvt_exchange_*


MERGE_SORTED_MAX_ROWS = (1 << 26) - 1   # include/nvt_hip.h nvt_count_merge_sorted
MERGE_SORTED_MAX_COLS = 64


IMAGE_LOOKUP_MAX_OUTPUTS = 24   # include/nvt_hip.h: nvt_flat_lookup_image, ncols <= 24


LOOKUP_IMAGES = os.environ.get("NVT_LOOKUP_IMAGES", "1") != "0"
# key -> group through the key directory (nvt_keydir_lookup_image: one 16-byte read per row, laid
# out by two small passes, no read-back) instead of the flat table ("0": nvt_flat_lookup_image)
KEYED_IMAGES = os.environ.get("NVT_KEYED_IMAGES", "1") != "0"
KEYDIR_LOAD = float(os.environ.get("NVT_KEYDIR_LOAD", "1.0"))   # keys per directory bucket
# records written whole by one launch over every operator's range (nvt_image_build); "0": a launch
# per operator (nvt_jg_image / nvt_te_image)
ONE_PASS_IMAGES = os.environ.get("NVT_ONE_PASS_IMAGES", "1") != "0"
# Workflow.fit ends by enqueueing the lookup images of its groupby operators (FlatIndex.prepare_image)
# instead of leaving them to the first transform; "0": built lazily by the first lookup.
EAGER_IMAGES = os.environ.get("NVT_EAGER_IMAGES", "1") != "0"

# ---- the rest of the driver lives beside this file; the facade re-exports it ---------------------
from .kernels_groupby import (  # noqa: E402,F401
    GroupbyTable, sorted_groupby_eligible, sorted_groupby, flat_index_for, te_apply_folds, _order_ws, order_rows, seg_aggregate, seg_nunique, gather, te_apply,
)
from .kernels_lookup import (  # noqa: E402,F401
    FlatIndex, _value_bits, LookupConsumer, image_pack, JG_KINDS, jg_image, jg_image_part, te_image_part, te_image,
)
from .kernels_exchange import (  # noqa: E402,F401
    ExchangeBatch, exchange_unpack, merge_counts_sorted,
)
from .kernels_encode import (  # noqa: E402,F401
    ENCODE_RESIDENT_I32, ENCODE_RESIDENT_I64, EncodeTable, encode_kind, encode_launch_shape, flat_tables_ok,
    encode_many, hash_bucket,
)
from .kernels_count import (  # noqa: E402,F401
    MIN_COUNT_CAPACITY, CountTable, count_into_new_table,
    PATH_S_MAX_DISTINCT, PATH_S_MAX_WEIGHTED, PATH_ORDER, _S_CLASSES, PATH_S2_FACTOR, PATH_P1_MAX_DISTINCT, PATH_P1_MAX_SMALL,
    PATH_P2_MAX_DISTINCT, PATH_P2_MAX_WEIGHTED, PATH_P3_MAX_DISTINCT, PATH_RANGE, PATH_PIECES, PATH_SORT, PATH_HOT,
    RANGE_AUX_WORDS, RANGE_AUX_HIST, RANGE_AUX_PW, RANGE_KEYS_PER_BUCKET, HOT_IMAGE_WORDS, SAMPLE_ROWS, SAMPLE_MIN_ROWS,
    _path_for, _path_max, CountPolicy, escalate, _launch_path_of, assign_streams, DenseCountJob, _estimate_distinct,
    _presample, CountBatch, dense_count_many, dense_count, merge_dense, merge_dense_many, CountMemory,
)
