// Categorify.transform / HashBucket on MI355X.
//
// Replaces the pandas `codes.merge(vocab, how="left").sort_values("order")`
// hash join + re-sort of categorify.py:1774-1776 (_encode) with one streaming
// pass: each lane loads 16 B of keys, probes a {key,label} open-addressing
// table and writes the labels with 16/32-byte stores.  Row order is preserved by
// construction, so the reference's O(n log n) re-sort disappears.
//
// Bytes per row (int32 keys, int64 labels): 4 read + 8 written = 12; the table
// probe is extra traffic that stays in L2 / Infinity Cache for all but the
// ~4e7-key columns.
//
// This unit holds the row kernels, the choice between them and the C entry points:
//   nvt_encode_table.hpp   slots, non-temporal accesses, the LDS head and its builder
//   nvt_encode_head.hpp    encode_small_kernel, encode_hot_kernel
//   nvt_encode_pipe.hpp    encode_pipe_kernel
// The tables are built by nvt_encode_build.hip; HashBucket is nvt_hash_bucket.hip.
#include <cstdlib>
#include <type_traits>

#include "nvt_common.hpp"
#include "nvt_encode_table.hpp"
#include "nvt_internal.hpp"
#include "nvt_prof.hpp"

namespace nvt {
// rows that went on to the table in HBM / rows looked up, when the host asks for them
// (NVT_ENC_STATS=1, nvt_encode_stats): a diagnostic, two atomics per wave at the kernel's end
__device__ unsigned long long g_enc_stats[2];

}  // namespace nvt

#include "nvt_encode_head.hpp"
#include "nvt_encode_pipe.hpp"

namespace nvt {

template <typename K>
__device__ __forceinline__ int64_t probe(const EncSlot<K> *__restrict__ table, uint64_t mask,
                                         K key) {
  constexpr K EMPTY = EncTraits<K>::empty;
  uint64_t slot = (uint64_t)slot_hash(key) & mask;
  while (true) {
    EncSlot<K> s = table[slot];
    if (s.key == key) return (int64_t)s.label;
    if (s.key == EMPTY) return -1;
    slot = (slot + 1) & mask;
  }
}

template <typename K, typename OUT>
__global__ __launch_bounds__(kBlock) void encode_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const EncSlot<K> *__restrict__ table, uint64_t mask, const int64_t *__restrict__ sentinel_label,
    int64_t null_label, int64_t oov_label, uint32_t num_buckets, OUT *__restrict__ out) {
  constexpr K EMPTY = EncTraits<K>::empty;
  constexpr int VEC = EncTraits<K>::vec;
  const int64_t sent = *sentinel_label;

  auto label_of = [&](K key, bool ok) -> OUT {
    if (!ok) return (OUT)null_label;
    int64_t lab = (key == EMPTY) ? sent : probe<K>(table, mask, key);
    if (lab < 0) {
      lab = oov_label;
      if (num_buckets > 1) lab += (int64_t)(key_hash32((int64_t)key) % num_buckets);
    }
    return (OUT)lab;
  };

  const uint64_t nvec = n / VEC;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
  const VecT *vkeys = reinterpret_cast<const VecT *>(keys);
  for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < nvec; v += stride) {
    VecT pack = vkeys[v];
    unsigned vbits = 0xF;
    if (valid != nullptr) {
      uint64_t row = v * VEC;
      vbits = (valid[row >> 3] >> (row & 7));
    }
    K k[VEC];
    if constexpr (sizeof(K) == 4) {
      k[0] = pack.x;
      k[1] = pack.y;
      k[2] = pack.z;
      k[3] = pack.w;
    } else {
      k[0] = pack.x;
      k[1] = pack.y;
    }
    OUT r[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) r[j] = label_of(k[j], (vbits >> j) & 1);
    // VEC * sizeof(OUT) is 8, 16 or 32 bytes: store as 1-2 wide vectors
    OUT *dst = out + v * VEC;
    if constexpr (VEC * sizeof(OUT) == 32) {
      int4 a, b;
      memcpy(&a, &r[0], 16);
      memcpy(&b, &r[2], 16);
      reinterpret_cast<int4 *>(dst)[0] = a;
      reinterpret_cast<int4 *>(dst)[1] = b;
    } else if constexpr (VEC * sizeof(OUT) == 16) {
      int4 a;
      memcpy(&a, &r[0], 16);
      reinterpret_cast<int4 *>(dst)[0] = a;
    } else {
      int2 a;
      memcpy(&a, &r[0], 8);
      reinterpret_cast<int2 *>(dst)[0] = a;
    }
  }
  for (uint64_t i = nvec * VEC + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    out[i] = label_of(keys[i], bit_valid(valid, i));
}

#ifndef NVT_HOT_DIV
#define NVT_HOT_DIV 4
#endif

// The launch shapes, under the names kernels_encode.py gives them (encode_launch_shape)
enum class EncShape {
  Generic,         // encode_kernel
  Small2048,       // encode_small_kernel<2048>
  Small4096,       // encode_small_kernel<4096>
  HotResident,     // encode_hot_kernel<GLOBAL=false>
  HotLinear64,     // encode_hot_kernel<int64,GLOBAL=true>
  CacheImage,      // cache mode, head image     } one kernel: its workgroups copy the prebuilt
  CachePerLaunch,  // cache mode, head per launch } head, or each builds it for itself
  Pipe2,           // encode_pipe_kernel<2>
  Pipe1,           // encode_pipe_kernel<1>
};

// ordered: the caller passed the frequency-ordered, duplicate-free vocabulary (vocab_keys, n_vocab > 0)
inline EncShape enc_shape_of(int key_bytes, int out_bytes, bool ordered, bool resident, uint64_t n_vocab,
                             bool range_table, uint64_t capacity, bool head_image) {
  if (!ordered) return EncShape::Generic;
  if (resident) {
    // small vocabularies with int64 labels: smaller tables, 256-thread workgroups, contiguous stores
    if (key_bytes == 4 && out_bytes == 8 && n_vocab <= 2048)
      return n_vocab <= 1024 ? EncShape::Small2048 : EncShape::Small4096;
    // fully staged (no global table) up to half load: linear probing of a table in which every
    // lookup hits stays short there (a 73 %-full table made an 11.9 k-key column 229 instead
    // of 129 us); larger vocabularies use the cache mode below
    return EncShape::HotResident;
  }
  // int64 keys: the linear-probing head filled to a quarter -- most lookups of it MISS, and an
  // unsuccessful linear probe costs ~2.5 slots at 50 % load but ~8.5 at 75 % (measured: 530 ->
  // 1290 us on a 6 M-key column)
  if (key_bytes == 8) return EncShape::HotLinear64;
  // cache mode: the 2-choice head filled to 7/8 (prebuilt as head_image when the caller has one);
  // rows that miss it go on to the table in HBM: a FLAT range table of `capacity` slots, the bucket
  // regions dumped by the counting pass (capacity 0), or the hashed table
  if (range_table) return capacity > 0 ? EncShape::Pipe2 : EncShape::Pipe1;
  return head_image ? EncShape::CacheImage : EncShape::CachePerLaunch;
}

// one column: the descriptor's fields are the arguments of nvt_encode_i32 / _i64
template <typename K>
int encode_launch(const nvt_encode_col &c, hipStream_t s) {
  constexpr bool k32 = sizeof(K) == 4;
  const K *keys = reinterpret_cast<const K *>(c.keys), *hot_keys = reinterpret_cast<const K *>(c.vocab_keys);
  // (range tables and head images belong to int32 keys: an int64 column's are not looked at)
  const int32_t *range_aux = k32 ? c.range_aux : nullptr;
  const auto *image = reinterpret_cast<const unsigned char *>(k32 ? c.head_image : nullptr);
  const uint64_t n = c.n, n_vocab = c.n_vocab, capacity = c.capacity, mask = capacity - 1;
  const int out_bytes = c.out_bytes;
  const bool ordered = hot_keys != nullptr && n_vocab > 0;
  // a duplicate-free vocabulary that fits the LDS table is encoded without the global table
  const bool resident = ordered && n_vocab <= (k32 ? NVT_ENCODE_RESIDENT_I32 : NVT_ENCODE_RESIDENT_I64);
  NVT_CHECK_ARG(resident || (c.table && c.sentinel_label), "null table");
  NVT_CHECK_ARG(resident || range_aux || (capacity >= 64 && (capacity & (capacity - 1)) == 0),
                "capacity must be 2^k >= 64");
  NVT_CHECK_ARG(range_aux == nullptr || (k32 && ordered),
                "range tables: int32 keys with the ordered vocabulary (vocab_keys)");
  NVT_CHECK_ARG(out_bytes == 4 || out_bytes == 8, "out_bytes must be 4 or 8");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(keys && c.out, "null keys/out");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(keys) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.out) & 15) == 0,
                "keys/out must be 16-byte aligned");
  const EncShape shape =
      enc_shape_of(sizeof(K), out_bytes, ordered, resident, n_vocab, range_aux != nullptr, capacity, image != nullptr);
  constexpr int VEC = EncTraits<K>::vec;
  auto *t = reinterpret_cast<const EncSlot<K> *>(c.table);
  NVT_PROF(k32 ? "encode_i32" : "encode_i64", n * (sizeof(K) + (uint64_t)out_bytes), s);
  // the launches below differ in the label type only: `launch` gets the typed output pointer
  auto with_out = [&](auto launch) {
    if (out_bytes == 8) launch(reinterpret_cast<int64_t *>(c.out));
    else launch(reinterpret_cast<int32_t *>(c.out));
  };
  // grid of the kernels that hold the head of the frequency-ordered vocabulary in LDS
  const unsigned hgrid = stream_grid(n / VEC + 1, kEncBS * 2, 1);
  static const int stats = getenv("NVT_ENC_STATS") ? atoi(getenv("NVT_ENC_STATS")) : 0;
  const uint32_t n_all = (uint32_t)n_vocab;   // (the resident shapes stage every key)
  const uint32_t n_hot = (uint32_t)(n_vocab < (uint64_t)kHead16Keys ? n_vocab : (uint64_t)kHead16Keys);
  with_out([&](auto *o) {
    using OUT = std::remove_pointer_t<decltype(o)>;
    switch (shape) {
      case EncShape::Generic:
        encode_kernel<K, OUT><<<stream_grid(n / VEC + 1, kBlock * 2, 8), kBlock, 0, s>>>(
            keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o);
        break;
      case EncShape::Small2048:
      case EncShape::Small4096:
        if constexpr (k32 && sizeof(OUT) == 8) {
          const unsigned sgrid = stream_grid(n / 2 + 1, kBlock * 8, 8);
          if (shape == EncShape::Small2048)
            encode_small_kernel<2048><<<sgrid, kBlock, 0, s>>>(keys, c.valid, n, c.null_label, c.oov_label,
                                                               c.num_buckets, o, hot_keys, n_all, c.first_label);
          else
            encode_small_kernel<4096><<<sgrid, kBlock, 0, s>>>(keys, c.valid, n, c.null_label, c.oov_label,
                                                               c.num_buckets, o, hot_keys, n_all, c.first_label);
        }
        break;
      case EncShape::HotResident:
        encode_hot_kernel<K, OUT, false, false><<<hgrid, kEncBS, 0, s>>>(
            keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o, hot_keys,
            n_all, c.first_label, 0, nullptr);
        break;
      case EncShape::HotLinear64:
        if constexpr (!k32)
          encode_hot_kernel<K, OUT, false, true><<<hgrid, kEncBS, 0, s>>>(
              keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o, hot_keys,
              (uint32_t)HotCfg<K>::slots / NVT_HOT_DIV, c.first_label, 0, nullptr);
        break;
      case EncShape::CacheImage:
      case EncShape::CachePerLaunch:
        if constexpr (k32)
          encode_hot_kernel<K, OUT, true, true><<<hgrid, kEncBS, 0, s>>>(
              keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o, hot_keys,
              n_hot, c.first_label, stats, image);
        break;
      case EncShape::Pipe2:   // (`mask` bounds the search)
        if constexpr (k32)
          encode_pipe_kernel<OUT, 2><<<hgrid, kEncBS, 0, s>>>(
              keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o, hot_keys,
              n_hot, c.first_label, range_aux, stats, image);
        break;
      case EncShape::Pipe1:   // (`mask` unused)
        if constexpr (k32)
          encode_pipe_kernel<OUT, 1><<<hgrid, kEncBS, 0, s>>>(
              keys, c.valid, n, t, mask, c.sentinel_label, c.null_label, c.oov_label, c.num_buckets, o, hot_keys,
              n_hot, c.first_label, range_aux, stats, image);
        break;
    }
  });
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_encode_stats(uint64_t *out2, int reset, void *stream) {
  NVT_CHECK_ARG(out2, "null out");
  hipStream_t s = (hipStream_t)stream;
  NVT_CHECK_HIP(hipStreamSynchronize(s));
  unsigned long long v[2] = {0, 0};
  NVT_CHECK_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_enc_stats), sizeof(v)));
  out2[0] = v[0];
  out2[1] = v[1];
  if (reset) {
    const unsigned long long z[2] = {0, 0};
    NVT_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_enc_stats), z, sizeof(z)));
  }
  return NVT_OK;
}

int nvt_encode_i32(const int32_t *keys, const uint8_t *valid, uint64_t n, const void *table,
                   uint64_t capacity, const int64_t *sentinel_label, int64_t null_label,
                   int64_t oov_label, uint32_t num_buckets, void *out, int out_bytes,
                   const int32_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                   void *stream) {
  const nvt_encode_col c = {keys, valid, n, table, capacity, sentinel_label, null_label, oov_label,
                            num_buckets, 4, out_bytes, out, vocab_keys, n_vocab, first_label};
  return encode_launch<int32_t>(c, (hipStream_t)stream);
}
int nvt_encode_i64(const int64_t *keys, const uint8_t *valid, uint64_t n, const void *table,
                   uint64_t capacity, const int64_t *sentinel_label, int64_t null_label,
                   int64_t oov_label, uint32_t num_buckets, void *out, int out_bytes,
                   const int64_t *vocab_keys, uint64_t n_vocab, int64_t first_label,
                   void *stream) {
  const nvt_encode_col c = {keys, valid, n, table, capacity, sentinel_label, null_label, oov_label,
                            num_buckets, 8, out_bytes, out, vocab_keys, n_vocab, first_label};
  return encode_launch<int64_t>(c, (hipStream_t)stream);
}
int nvt_encode_many(const nvt_encode_col *cols, int ncols, void *stream) {
  NVT_CHECK_ARG(ncols == 0 || cols, "null descriptors");
  // the columns are independent (own output, own tables): they go round-robin onto
  // NVT_ENCODE_STREAMS (default 3) internal streams forked from / joined into `stream`.  Round 2
  // measured nothing for it (15.42 / 15.40 / 15.31 ms per step with 1 / 2 / 3 streams: every encode
  // kernel filled the chip with one 128 KiB-LDS workgroup per CU and was bound by the HBM stream for
  // its whole duration); the pipelined cache mode of round 6 waits for table probes for a good part
  // of its launches and leaves stream bandwidth to the launch beside it: 9.55 / 9.25 / 9.20 / 9.20 ms
  // per step with 1 / 2 / 3 / 4 streams.  (Read at every call: bench.py's per-kernel pass sets 1.)
  const int n_side = [] {
    const char *e = getenv("NVT_ENCODE_STREAMS");
    int v = e ? atoi(e) : 3;
    return v < 1 ? 1 : v > kSideStreams ? kSideStreams : v;
  }();
  hipStream_t main_s = (hipStream_t)stream;
  SidePool *pool = nullptr;
  const int lanes = ncols < n_side ? ncols : n_side;
  const bool fork = lanes > 1;
  if (fork) {
    int rc = side_pool(2, &pool);
    if (rc) return rc;
    NVT_CHECK_HIP(hipEventRecord(pool->fork, main_s));
    for (int k = 0; k < lanes; ++k) NVT_CHECK_HIP(hipStreamWaitEvent(pool->s[k], pool->fork, 0));
  }
  int rc_all = NVT_OK;
  for (int i = 0; i < ncols; ++i) {
    const nvt_encode_col &c = cols[i];
    hipStream_t cs = fork ? pool->s[i % lanes] : main_s;
    int rc;
    if (c.wait_event) NVT_CHECK_HIP(hipStreamWaitEvent(cs, (hipEvent_t)c.wait_event, 0));
    if (c.key_bytes == 4)
      rc = encode_launch<int32_t>(c, cs);
    else if (c.key_bytes == 8)
      rc = encode_launch<int64_t>(c, cs);
    else {
      set_error("nvt_encode_many: key_bytes must be 4 or 8 (column %d)", i);
      rc = NVT_EINVAL;
    }
    if (rc) {
      rc_all = rc;  // (the internal streams are joined below all the same)
      break;
    }
  }
  if (fork)
    for (int k = 0; k < lanes; ++k) {
      NVT_CHECK_HIP(hipEventRecord(pool->join[k], pool->s[k]));
      NVT_CHECK_HIP(hipStreamWaitEvent(main_s, pool->join[k], 0));
    }
  return rc_all;
}

}  // extern "C"
