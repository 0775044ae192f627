"""The encode driver of Categorify.transform: EncodeTable (the key -> label table of one
vocabulary, whichever form it takes), nvt_vocab_finalize_many / nvt_encode_many descriptors,
HashBucket, and the policy that says which kind of table a vocabulary gets and which kernel
encodes with it.

The policy is pure: ``encode_kind`` (the kind of table) and ``encode_launch_shape`` (the kernel
``encode_launch`` of csrc/nvt_encode.hip picks, under the names of its ``EncShape``) touch neither
torch nor the library, and tests/test_host_logic.py pins them.

Part of the host driver of the C ABI (include/nvt_hip.h); ``kernels.py`` is the facade every
caller imports -- it re-exports these names, holds the run-time switches they read (``K.<FLAG>`` at
call time: tests and A / B runs set them on the facade) and the helpers they share."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib
from . import kernels as K
from ._lib import check

# a duplicate-free vocabulary of at most this many keys is encoded from LDS alone: no global table,
# no build kernel (include/nvt_hip.h NVT_ENCODE_RESIDENT_*).  Re-exported by the facade and read
# there (``K.ENCODE_RESIDENT_*``) like the switches: a test lifts the gate on ``K``
ENCODE_RESIDENT_I32, ENCODE_RESIDENT_I64 = 8192, 6144
_BYTES = {}   # (size function of the library, its arguments) -> bytes


def encode_kind(key_bytes: int, n_vocab: int, unique: bool, defer_build: bool, has_range_table: bool,
                flat: bool) -> str:
    """The kind of table EncodeTable makes; first match wins.

    resident   the whole vocabulary is staged in LDS by every launch: no table at all
    dumped     the range table the counting pass dumped, completed by nvt_vocab_finalize_many
    flat       a flat range table laid out from the key-sorted source by nvt_vocab_finalize_many
    cache      hashed table, int32 keys; the head of the ordered vocabulary in LDS in front of it
    linear64   the same with int64 keys (linear-probing head)
    generic    hashed table alone: duplicate keys (user-supplied vocabularies) or no keys"""
    resident = K.ENCODE_RESIDENT_I32 if key_bytes == 4 else K.ENCODE_RESIDENT_I64
    if unique and 0 < n_vocab <= resident:
        return "resident"
    if has_range_table:
        assert defer_build and unique and key_bytes == 4
        return "dumped"
    if flat and defer_build and unique and key_bytes == 4:
        return "flat"
    if unique and n_vocab > 0:
        return "cache" if key_bytes == 4 else "linear64"
    return "generic"


def encode_launch_shape(kind: str, key_bytes: int, out_bytes: int, n_vocab: int, has_head_image: bool) -> str:
    """The kernel instantiation a table of ``kind`` is encoded with (csrc/nvt_encode.hip: EncShape)."""
    if kind == "generic":
        return "encode_kernel"
    if kind == "resident":
        if key_bytes == 4 and out_bytes == 8 and n_vocab <= 2048:
            return "encode_small_kernel<2048>" if n_vocab <= 1024 else "encode_small_kernel<4096>"
        return "encode_hot_kernel<GLOBAL=false>"
    if kind == "linear64":
        return "encode_hot_kernel<int64,GLOBAL=true>"
    if kind in ("flat", "dumped"):
        return "encode_pipe_kernel<2>" if kind == "flat" else "encode_pipe_kernel<1>"
    return "cache mode, head image" if has_head_image else "cache mode, head per launch"


def _lib_bytes(name: str, *args) -> int:
    key = (name,) + args
    if key not in _BYTES:
        out = C.c_uint64()
        check(getattr(_lib.load(), name)(*args, C.byref(out)), name)
        _BYTES[key] = out.value
    return _BYTES[key]


SMALL_SORT_CHUNK = 2048   # csrc/nvt_sort.hip kSmallChunk: lists up to here need no sort scratch


class EncodeTable:
    """key -> label probe table built from an ordered vocabulary."""

    FLAT_AUX_WORDS, FLAT_AUX_MAXDISP = 8192 + 16, 8192 + 8   # include/nvt_hip.h NVT_FLAT_AUX_*
    FLAT_MAX_DISPLACEMENT = 4096   # longer probe runs than this: the keys cluster, use a hashed table

    def __init__(self, vocab_keys: torch.Tensor, first_label: int, unique: bool = False,
                 defer_build: bool = False, range_table=None, flat: bool = False):
        """range_table = (table, aux, bits[, slots]): the table was dumped by the range path of the
        counting stage and is addressed by the monotone map stored in ``aux``; it is completed
        (positions -> labels) by nvt_vocab_finalize_many -- no table is allocated or built here.
        ``slots`` (int32 per entry of the key-sorted list that the same counting pass emitted, or
        None): the table slot of every entry, through which the ordering writes the labels."""
        _lib.require_gpu()
        self.suffix = K._key_suffix(vocab_keys)
        self.key_dtype = vocab_keys.dtype
        self.key_bytes = 4 if self.suffix == "i32" else 8
        self.n_vocab = n = int(vocab_keys.numel())
        self.first_label = int(first_label)
        self.unique = bool(unique)
        self.kind = kind = encode_kind(self.key_bytes, n, self.unique, bool(defer_build),
                                       range_table is not None, bool(flat))
        dev = vocab_keys.device
        self._vk = vk = vocab_keys.contiguous()
        # kept: the head of the (frequency-ordered, duplicate-free) vocabulary is staged in LDS
        self.vocab_keys = vk if unique else None
        self.sort_tmp = None
        self._counts = None    # the counts tensor while an internal stream still orders it
        self._src = None       # key-sorted source list of the one-pass ordering, same lifetime
        self.ready = None      # Event recorded behind the sort / build on an internal stream
        self.pending = False   # True until the current stream has been made to wait for it
        self._release = False  # True between fill_encode_desc and release_ordering (encode_many)
        self.table = self.range_aux = self.range_slots = None
        self.range_bits = self.flat_slots = 0
        self.capacity = K.next_pow2(max(64, (4 if n <= (1 << 20) else 2) * n + 1))   # hashed tables
        hashed = kind in ("generic", "cache", "linear64")
        if kind == "dumped":
            self.table, self.range_aux, self.range_bits = range_table[:3]
            self.range_slots = range_table[3] if len(range_table) > 3 else None
            self.capacity = 0
        elif kind == "flat":
            # flat range table laid out from the key-sorted source by nvt_vocab_finalize_many
            # (prefix maximum, no random inserts): 2^k >= 2 n slots + n + 64 tail slots
            # home slots at load FLAT_INDEX_LOAD (no power of two: 36 M keys took 2^27 slots = 1 GiB
            # to clear and fill, now 576 MB)
            self.flat_slots = max(64, int(n / K.FLAT_INDEX_LOAD) + 1)
            self.capacity = self.flat_slots + n + 64
            self.table = torch.empty(self.capacity * 8, dtype=torch.uint8, device=dev)
            self.range_aux = torch.empty(self.FLAT_AUX_WORDS, dtype=torch.int32, device=dev)
        elif hashed:
            nbytes = _lib_bytes("nvt_encode_table_bytes", self.key_bytes, self.capacity)
            self.table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # (the label of the smallest key of the type, which marks the empty slots of every table)
        self.sentinel_label = None if kind == "resident" else torch.empty(1, dtype=torch.int64, device=dev)
        # the LDS head of the cache-mode encode, built ONCE per vocabulary by
        # nvt_vocab_finalize_many (include/nvt_hip.h nvt_vocab_col.head_image): only tables whose
        # vocabulary is ordered there (defer_build) get one
        self.head_image = None
        if defer_build and kind in ("cache", "flat", "dumped"):
            self.head_image = torch.empty(_lib.ENCODE_HEAD_BYTES, dtype=torch.uint8, device=dev)
        if hashed and not defer_build:  # (deferred: built by nvt_vocab_finalize_many, after the ordering)
            check(
                getattr(_lib.load(), f"nvt_encode_build_{self.suffix}")(
                    vk.data_ptr() if n else None, n, self.first_label, self.table.data_ptr(),
                    self.capacity, self.sentinel_label.data_ptr(), 1 if unique else 0, K.stream_ptr(),
                ),
                "nvt_encode_build",
            )

    def fill_vocab_desc(self, d: "_lib.VocabCol", counts: torch.Tensor, max_count: int, src=None):
        """One nvt_vocab_col: order (self vocab keys, counts) in place, then build the table.
        ``src`` = (keys, counts, cls_hist, n_big) of a KEY-SORTED list (range path): the
        vocabulary is then written out of place into (self vocab keys, counts) by one stable
        counting pass that also fills the table."""
        n = self.n_vocab
        src_keys = src_counts = cls_hist = labels = None
        n_big = small_scratch = 0
        if src is not None:
            src_keys, src_counts, cls_hist, n_big = src[:4]
            # (a fifth element: int32 positions of the source entries in the vocabulary order -- a
            # multi-GPU fit whose owners labelled their shards; no ordering pass is run then)
            labels = src[4] if len(src) > 4 else None
            if labels is not None:
                assert labels.dtype == torch.int32 and labels.numel() == src_keys.numel()
                labels, n_big = labels.contiguous(), 0
                K.stat_add("labelled_vocabularies")
            assert self.key_bytes == 4 and self.unique and src_keys.numel() == n and counts.numel() == n
            self._src = (src_keys, src_counts, cls_hist, labels)  # read on an internal stream until `ready`
            scratch = _lib_bytes("nvt_vocab_order_tmp_bytes", n, int(n_big))
        else:
            small = self.key_bytes == 4 and 2 <= n <= 16384 and 0 < int(max_count) < (1 << 32)
            scratch = _lib_bytes("nvt_vocab_sort_tmp_bytes", self.key_bytes, n) if n > 1 and not small else None
            if small and n > SMALL_SORT_CHUNK:
                # the batched small sort merges the sorted chunks of a longer list through 8 n bytes;
                # it runs on the caller's stream, so no hand-off event goes with this scratch
                small_scratch = 8 * n
        # the counts are ordered in place on the same internal stream as the keys: they must
        # outlive the hand-off event exactly like keys / table / sort_tmp (a rank that writes
        # no artifacts used to drop its only reference right after the launch)
        self._counts = counts
        d.keys = self._vk.data_ptr()
        d.counts = counts.data_ptr()
        d.n = n
        d.max_count = int(max_count)
        d.key_bytes = self.key_bytes
        d.unique_keys = 1 if self.unique else 0
        d.src_keys, d.src_counts = K.ptr(src_keys), K.ptr(src_counts)
        d.cls_hist, d.src_labels = K.ptr(cls_hist), K.ptr(labels)
        d.src_slots = None
        if self.range_slots is not None and src is not None and labels is None:
            assert self.range_slots.dtype == torch.int32 and self.range_slots.numel() == n
            d.src_slots = self.range_slots.data_ptr()
        d.n_big = int(n_big)
        d.range_aux = K.ptr(self.range_aux)
        d.range_nb_log2 = int(self.range_bits)
        d.flat_slots = int(self.flat_slots)
        if scratch is not None:
            self.sort_tmp = torch.empty(scratch + 16, dtype=torch.uint8, device=self._vk.device)
        elif small_scratch:
            self.sort_tmp = torch.empty(small_scratch + 16, dtype=torch.uint8, device=self._vk.device)
        d.sort_tmp = K.ptr(self.sort_tmp) if scratch is not None or small_scratch else None
        d.first_label = self.first_label
        d.table = K.ptr(self.table)
        d.capacity = self.capacity
        d.sentinel_label = K.ptr(self.sentinel_label)
        d.head_image = K.ptr(self.head_image)
        if scratch is not None and K.ASYNC_FINALIZE:
            # ordered on an internal stream: hand-off by event instead of a stream join, so the
            # caller's stream keeps working (fill + normalize, encodes of the small vocabularies)
            # underneath this vocabulary's radix passes and table build
            if self.ready is None:
                self.ready = K.Event()
            d.ready_event = self.ready.handle
            self.pending = True
        else:
            d.ready_event = None

    def flat_ok(self) -> bool:
        """Flat range tables only: True when no entry sits further than FLAT_MAX_DISPLACEMENT slots
        from its home slot.  Synchronises (the finalisation of this vocabulary has to be done)."""
        self.wait_ready()
        return int(self.range_aux[self.FLAT_AUX_MAXDISP].item()) & 0xFFFFFFFF <= self.FLAT_MAX_DISPLACEMENT

    def _drop_ordering(self):
        """Lets go of what the ordering of the vocabulary used (its scratch, the counts, the
        key-sorted source): the caller knows that the current stream is ordered behind it."""
        self.sort_tmp = None
        self._counts = None
        self._src = None
        self.range_slots = None

    def wait_ready(self):
        """Order the CURRENT stream behind this vocabulary's sort / table build (no host
        synchronisation).  Every consumer of the vocabulary or the table calls this first."""
        if self.pending:
            self.ready.wait()
            self.pending = False
            self._drop_ordering()  # scratch of the finished sort: safe to recycle from here on

    def __del__(self):
        try:
            if getattr(self, "pending", False):
                self.wait_ready()  # the buffers are about to be recycled on this stream
        except Exception:
            pass

    def fill_encode_desc(self, d: "_lib.EncodeCol", keys, valid, null_label, oov_label,
                         num_buckets, out):
        d.keys = keys.data_ptr()
        d.valid = K.ptr(valid)
        d.n = keys.numel()
        d.table = K.ptr(self.table)
        d.capacity = self.capacity
        d.sentinel_label = K.ptr(self.sentinel_label)
        d.null_label = int(null_label)
        d.oov_label = int(oov_label)
        d.num_buckets = int(num_buckets or 0)
        d.key_bytes = self.key_bytes
        d.out_bytes = out.element_size()
        d.out = out.data_ptr()
        d.vocab_keys = K.ptr(self.vocab_keys) if self.n_vocab else None
        d.n_vocab = self.n_vocab if self.vocab_keys is not None else 0
        d.first_label = self.first_label
        d.range_aux = K.ptr(self.range_aux)
        d.head_image = K.ptr(self.head_image)
        if self.pending:
            # nvt_encode_many waits on the launch stream.  The ordering's buffers are let go by
            # release_ordering(), AFTER that call is enqueued: dropped here, a block as large as a
            # label column (the n + 1 entry list of the sort path) went straight to the `out` of
            # the next column, whose encode waits for its OWN vocabulary only and wrote its labels
            # over the counts this vocabulary's ordering pass was still reading
            d.wait_event = self.ready.handle
            self.pending = False
            self._release = True
        else:
            d.wait_event = None

    def release_ordering(self):
        """Behind nvt_encode_many (which joined its streams into the launch stream, each behind
        the ready events it was given): the scratch of the finished ordering may be recycled."""
        if self._release:
            self._release = False
            self._drop_ordering()

    def encode(self, keys: torch.Tensor, valid: Optional[torch.Tensor], null_label: int, oov_label: int,
               num_buckets: int = 0, out_dtype: torch.dtype = torch.int64) -> torch.Tensor:
        """One column through encode_many: with one column nvt_encode_many forks no streams and
        waits for this table's event on the current stream."""
        return encode_many([(self, keys, valid, null_label, oov_label, num_buckets)], out_dtype)[0]


def flat_tables_ok(tabs) -> List[bool]:
    """EncodeTable.flat_ok for several flat range tables with ONE read-back, taken on a side
    stream that waits for nothing but the tables' own finalisation events: work already queued on
    the current stream (the encodes that use these very tables) is neither waited for by the host
    nor held up on the device.  The tables must have been finalised with a ready event."""
    dev = tabs[0].range_aux.device
    side = K._check_streams.get(dev.index)
    if side is None:
        side = K._check_streams[dev.index] = torch.cuda.Stream(device=dev)
    for t in tabs:
        if t.ready is not None:
            t.ready.wait(stream=side.cuda_stream)
        else:
            side.wait_stream(torch.cuda.current_stream(dev))  # finalised on the caller's stream
    with torch.cuda.stream(side):
        words = torch.stack([t.range_aux[EncodeTable.FLAT_AUX_MAXDISP] for t in tabs]).to(torch.int64)
        vals = K.read_back(words)
    return [(int(d) & 0xFFFFFFFF) <= EncodeTable.FLAT_MAX_DISPLACEMENT for d in vals]


def encode_many(items, out_dtype: torch.dtype = torch.int64):
    """items: [(EncodeTable, keys, valid, null_label, oov_label, num_buckets)] -> [labels];
    every column of a Categorify.transform enqueued by ONE C call (nvt_encode_many)."""
    if out_dtype not in (torch.int32, torch.int64):
        raise TypeError("Categorify output dtype must be int32 or int64")
    # vocabularies still being ordered on an internal stream go last, largest first (the order
    # nvt_vocab_finalize_many works through them): everything that is ready runs underneath
    order = sorted(range(len(items)),
                   key=lambda i: (1, -items[i][0].n_vocab) if items[i][0].pending else (0, 0))
    descs = (_lib.EncodeCol * max(1, len(items)))()
    outs, keep = [None] * len(items), []
    for d, i in zip(descs, order):
        tab, keys, valid, null_label, oov_label, nb = items[i]
        if keys.dtype != tab.key_dtype:
            keys = keys.to(tab.key_dtype)
        keys = K.aligned(keys)
        out = torch.empty(keys.numel(), dtype=out_dtype, device=keys.device)
        tab.fill_encode_desc(d, keys, valid, null_label, oov_label, nb, out)
        outs[i] = out
        keep.append(keys)
    try:
        if items:
            check(_lib.load().nvt_encode_many(descs, len(items), K.stream_ptr()), "nvt_encode_many")
    finally:
        for it in items:
            it[0].release_ordering()
    return outs


def hash_bucket(
    keys: torch.Tensor,
    num_buckets: int,
    xor_in: Optional[torch.Tensor] = None,
    want_hash: bool = False,
    want_bucket: bool = True,
    valid: Optional[torch.Tensor] = None,
):
    """(bucket int32 or None, hash64 or None).  hash64 is carried as int64 bits.  Rows whose
    ``valid`` bit is clear hash as key 0 (the slot under a null holds arbitrary bytes)."""
    lib = _lib.load()
    _lib.require_gpu()
    keys = K.aligned(keys)
    n = keys.numel()
    out = torch.empty(n, dtype=torch.int32, device=keys.device) if want_bucket else None
    xo = torch.empty(n, dtype=torch.int64, device=keys.device) if want_hash else None
    check(
        getattr(lib, f"nvt_hash_bucket_{K._key_suffix(keys)}")(
            keys.data_ptr(), K.ptr(valid), n, int(num_buckets), K.ptr(out), K.ptr(xor_in), K.ptr(xo),
            K.stream_ptr()
        ),
        "nvt_hash_bucket",
    )
    return out, xo
