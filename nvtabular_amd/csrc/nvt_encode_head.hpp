// Row kernels that look every key up in an LDS table first: encode_small_kernel (the whole
// vocabulary in a 16 / 32 KiB table) and encode_hot_kernel (the whole vocabulary, or its head in
// front of the hashed table in HBM).  Bodies only, included by nvt_encode.hip: the library is
// built without relocatable device code, and encode_hot_kernel adds into that unit's g_enc_stats
// (defined in front of this include).
#pragma once
#include <type_traits>

#include "nvt_encode_table.hpp"

namespace nvt {

// Encode with the head of the vocabulary staged in LDS.  The vocabulary is ordered by
// frequency (categorify.py:1316), so its first entries are exactly the keys most rows
// carry: each workgroup copies the first n_hot entries into a private LDS table and only
// rows that miss it go to the global table in HBM.  A vocabulary that fits entirely
// (n_vocab <= n_hot) never touches the global table: pure stream + LDS gathers.
// The key and label streams of encode_hot_kernel are touched once; marking them non-temporal
// keeps the probe table (up to ~130 MB for a 6 M-key vocabulary) resident in L2 / Infinity Cache.
// Small vocabularies (<= SLOTS / 2 keys, int32 keys -> int64 labels: the reference's default dtype):
// the 4-in / 8-out stream of widen_stream (nvt_cont.hip) with an LDS lookup in the middle.  The
// fully staged encode_hot_kernel holds a 128 KiB table whatever the vocabulary, i.e. ONE 1024-thread
// workgroup per CU, and a lane that loads 16 bytes of keys owns 32 bytes of labels, written as two
// 16-byte stores 32 bytes apart: 131 us per 45 M-row column = 4.1 TB/s, of which experiment modes
// attribute 49 us to the stores, 48 us to the bare loop over the keys (3.75 TB/s with nothing but
// loads: 16 waves per CU) and 4 us to the lookups.  Here the table has SLOTS slots (16 / 32 KiB), a
// workgroup is 256 threads (8 / 5 of them per CU), a lane takes two keys per run of 128 and every
// store instruction of a wave covers 1024 contiguous bytes.
template <int SLOTS>
__global__ __launch_bounds__(kBlock) void encode_small_kernel(
    const int32_t *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n, int64_t null_label,
    int64_t oov_label, uint32_t num_buckets, int64_t *__restrict__ out,
    const int32_t *__restrict__ hot_keys, uint32_t n_hot, int64_t first_label) {
  constexpr int32_t EMPTY = EncTraits<int32_t>::empty;
  __shared__ EncSlot<int32_t> lt[SLOTS];
  __shared__ long long s_sent;
  for (int i = threadIdx.x; i < SLOTS; i += kBlock) {
    lt[i].key = EMPTY;
    lt[i].label = 0;
  }
  if (threadIdx.x == 0) s_sent = -1;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_hot; i += kBlock) {
    const int32_t key = hot_keys[i];
    if (key == EMPTY) {
      s_sent = first_label + (long long)i;
      continue;
    }
    uint32_t sl = lds_home<SLOTS>(key);
    while (true) {
      const int32_t prev = atomicCAS(&lt[sl].key, EMPTY, key);
      if (prev == EMPTY || prev == key) {
        if (prev == EMPTY) lt[sl].label = (int32_t)(first_label + (int64_t)i);
        break;
      }
      sl = (sl + 1) & (SLOTS - 1);
    }
  }
  __syncthreads();
  const int64_t sent = (int64_t)s_sent;
  auto encode = [&](int32_t key, bool ok) -> int64_t {
    if (!ok) return null_label;
    int64_t lab = -1;
    if (key == EMPTY) {
      lab = sent;
    } else {
      uint32_t sl = lds_home<SLOTS>(key);
      while (true) {
        const EncSlot<int32_t> e = lt[sl];
        if (e.key == key) {
          lab = (int64_t)e.label;
          break;
        }
        if (e.key == EMPTY) break;
        sl = (sl + 1) & (SLOTS - 1);
      }
    }
    if (lab < 0) {
      lab = oov_label;
      if (num_buckets > 1) lab += (int64_t)(key_hash32((int64_t)key) % num_buckets);
    }
    return lab;
  };
  constexpr int RUN = 2 * kWave, U = 4;
  typedef int v2i_nt __attribute__((ext_vector_type(2)));
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const unsigned lane = threadIdx.x & (kWave - 1);
  const uint64_t nruns = n / RUN;
  // (the wave index through readfirstlane: run numbers, bounds and base addresses are scalar)
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) +
                        (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t nwaves = stride / kWave;
  for (uint64_t r0 = wave * U; r0 < nruns; r0 += nwaves * U) {
    v2i_nt raw[U];
    unsigned vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      raw[u] = v2i_nt{0, 0};
      vb[u] = 3u;
      if (r0 + u < nruns) {
        const uint64_t e = (r0 + u) * RUN + 2 * lane;
        raw[u] = __builtin_nontemporal_load(reinterpret_cast<const v2i_nt *>(keys + e));
        if (valid != nullptr) vb[u] = (unsigned)valid[e >> 3] >> (e & 7);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (r0 + u >= nruns) break;
      const uint64_t e = (r0 + u) * RUN + 2 * lane;
      int64_t r[2];
      r[0] = encode(raw[u].x, (bool)(vb[u] & 1));
      r[1] = encode(raw[u].y, (bool)((vb[u] >> 1) & 1));
      nvt_v4i o;
      memcpy(&o, r, 16);
      __builtin_nontemporal_store(o, reinterpret_cast<nvt_v4i *>(out + e));
    }
  }
  for (uint64_t i = nruns * RUN + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    out[i] = encode(keys[i], bit_valid(valid, i));
}

// GLOBAL = false: the whole vocabulary is staged (no table in HBM): the probe phases and their
// registers disappear.  (3 / 4 key vectors per lane in flight instead of U = 2, and a 2048-slot
// table with two workgroups per CU for vocabularies <= 1024 keys, were each ~2 % slower:
// profiles/r02_notes.md)
// TWO: cache mode of int32 keys with a hashed table in HBM (range tables go to encode_pipe_kernel).
template <typename K, typename OUT, bool TWO = false, bool GLOBAL = true>
__global__ __launch_bounds__(kEncBS, 1) void encode_hot_kernel(
    const K *__restrict__ keys, const uint8_t *__restrict__ valid, uint64_t n,
    const EncSlot<K> *__restrict__ table, uint64_t mask, const int64_t *__restrict__ sentinel_label,
    int64_t null_label, int64_t oov_label, uint32_t num_buckets, OUT *__restrict__ out,
    const K *__restrict__ hot_keys, uint32_t n_hot, int64_t first_label, int count_stats,
    const unsigned char *__restrict__ head_image) {
  static_assert(!TWO || (GLOBAL && sizeof(K) == 4), "TWO: the 2-choice head of int32 keys in cache mode");
  constexpr bool global_needed = GLOBAL;
  constexpr K EMPTY = EncTraits<K>::empty;
  constexpr int VEC = EncTraits<K>::vec;
  constexpr int SLOTS = HotCfg<K>::slots;
  constexpr int kLdsBytes = kHeadLdsBytes<K, TWO>;
  __shared__ __align__(16) unsigned char lraw[kLdsBytes];
  EncSlot<K> *lt = reinterpret_cast<EncSlot<K> *>(lraw);
  int2 *tkeys = reinterpret_cast<int2 *>(lraw);                                 // TWO: {key0, key1}
  uint32_t *tlab = reinterpret_cast<uint32_t *>(lraw + kHead16Buckets * 8);     // TWO: two 16-bit ranks
  __shared__ long long s_sent;  // label of the sentinel key when it is among the staged keys
  if (head_image != nullptr) {   // (uniform) prebuilt by nvt_vocab_finalize_many: coalesced copy
    const int4 *src = reinterpret_cast<const int4 *>(head_image);
    int4 *dst = reinterpret_cast<int4 *>(lraw);
    for (int i = threadIdx.x; i < kLdsBytes / 16; i += kEncBS) dst[i] = src[i];
    if (threadIdx.x == 0) s_sent = *reinterpret_cast<const long long *>(head_image + kLdsBytes);
    __syncthreads();
  } else {
    build_head<K, TWO>(lraw, &s_sent, hot_keys, n_hot, first_label);
  }
  // a vocabulary staged in full needs neither the global table nor its sentinel word
  const int64_t sent = global_needed ? *sentinel_label : (int64_t)s_sent;

  // LDS lookup: label, or -1 when the key is not in the staged head of the vocabulary
  auto hot_lookup = [&](K key) -> int64_t {
    if constexpr (TWO) {
      uint32_t b1, b2;
      two_buckets16((int32_t)key, b1, b2);
      const int2 a = tkeys[b1], c = tkeys[b2];
      const uint32_t la = tlab[b1], lc = tlab[b2];
      int lab = -1;
      lab = a.x == (int)key ? (int)(la & 0xFFFFu) : lab;
      lab = a.y == (int)key ? (int)(la >> 16) : lab;
      lab = c.x == (int)key ? (int)(lc & 0xFFFFu) : lab;
      lab = c.y == (int)key ? (int)(lc >> 16) : lab;
      return lab < 0 ? (int64_t)-1 : first_label + (int64_t)lab;
    }
    uint32_t s = lds_home<SLOTS>(key);
    while (true) {
      EncSlot<K> e = lt[s];
      if (e.key == key) return (int64_t)e.label;
      if (e.key == EMPTY) return -1;
      s = (s + 1) & (SLOTS - 1);
    }
  };
  auto finish = [&](K key, int64_t lab) -> OUT {
    if (lab < 0) {
      lab = oov_label;
      if (num_buckets > 1) lab += (int64_t)(key_hash32((int64_t)key) % num_buckets);
    }
    return (OUT)lab;
  };

  const uint64_t nvec = n / VEC;
  const uint64_t stride = (uint64_t)gridDim.x * kEncBS;
  using VecT = typename std::conditional<sizeof(K) == 4, int4, longlong2>::type;
  const VecT *vkeys = reinterpret_cast<const VecT *>(keys);
  constexpr int U = 2;  // key vectors per lane in flight
  constexpr int NK = U * VEC;
  // software pipeline: the key vectors (and bitmap bytes) of iteration i+1 are requested
  // before iteration i is processed -- with one 1024-thread workgroup per CU the stream
  // latency is otherwise exposed once per iteration (~20 iterations per column)
  VecT nxt_pack[U];
  unsigned nxt_vb[U];
  unsigned st_miss = 0, st_rows = 0;   // (count_stats)
  auto issue_loads = [&](uint64_t v0, VecT (&pk)[U], unsigned (&bits)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint64_t v = v0 + (uint64_t)u * stride;
      bits[u] = 0;
      if (v < nvec) {
        pk[u] = nt_load16(&vkeys[v]);
        bits[u] = 0x10000u | (valid ? (unsigned)valid[(v * VEC) >> 3] : 0xFFu);  // raw byte
      }
    }
  };
  issue_loads((uint64_t)blockIdx.x * kEncBS + threadIdx.x, nxt_pack, nxt_vb);
  for (uint64_t v0 = (uint64_t)blockIdx.x * kEncBS + threadIdx.x; v0 < nvec; v0 += stride * U) {
    VecT pack[U];
    unsigned vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pack[u] = nxt_pack[u];
      vb[u] = nxt_vb[u];
    }
    issue_loads(v0 + stride * U, nxt_pack, nxt_vb);
#pragma unroll
    for (int u = 0; u < U; ++u)  // shift after ALL loads are in flight (no early s_waitcnt)
      if (vb[u])
        vb[u] = 0x100u | (((vb[u] & 0xFFu) >> (((v0 + (uint64_t)u * stride) * VEC) & 7)) &
                          ((1u << VEC) - 1u));
    K k[NK];
    int64_t lab[NK];
    bool need[NK];  // still unresolved: must probe the table in HBM
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (sizeof(K) == 4) {
        k[u * VEC + 0] = pack[u].x;
        k[u * VEC + 1] = pack[u].y;
        k[u * VEC + 2] = pack[u].z;
        k[u * VEC + 3] = pack[u].w;
      } else {
        k[u * VEC + 0] = pack[u].x;
        k[u * VEC + 1] = pack[u].y;
      }
    }
    // phase 1: LDS
#pragma unroll
    for (int q = 0; q < NK; ++q) {
      const bool ok = (vb[q / VEC] & 0x100) && ((vb[q / VEC] >> (q % VEC)) & 1);
      lab[q] = -1;
      need[q] = false;
      if (ok) {
        if (k[q] == EMPTY) {
          lab[q] = sent;
        } else {
          lab[q] = hot_lookup(k[q]);
          need[q] = lab[q] < 0 && global_needed;
          if (count_stats) {
            st_rows += 1u;
            st_miss += need[q] ? 1u : 0u;
          }
        }
      } else {
        lab[q] = null_label;
      }
    }
    // phase 2: first probe of every miss issued back to back (independent loads), so the
    // HBM / Infinity-Cache latency is paid once per batch, not once per key
    if constexpr (GLOBAL) {
      uint64_t slot[NK];
      EncSlot<K> e[NK];
#pragma unroll
      for (int q = 0; q < NK; ++q) {
        slot[q] = (uint64_t)slot_hash(k[q]) & mask;
        if (need[q]) e[q] = table[slot[q]];
      }
#pragma unroll
      for (int q = 0; q < NK; ++q) {
        if (!need[q]) continue;
        while (true) {  // collisions continue here (load factor <= 0.5: short chains)
          if (e[q].key == k[q]) {
            lab[q] = (int64_t)e[q].label;
            break;
          }
          if (e[q].key == EMPTY) break;
          slot[q] = (slot[q] + 1) & mask;
          e[q] = table[slot[q]];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!(vb[u] & 0x100)) continue;
      uint64_t v = v0 + (uint64_t)u * stride;
      OUT r[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int q = u * VEC + j;
        const bool ok = (vb[u] >> j) & 1;
        r[j] = ok ? finish(k[q], lab[q]) : (OUT)null_label;
      }
      OUT *dst = out + v * VEC;
      if constexpr (VEC * sizeof(OUT) == 32) {
        int4 a, b;
        memcpy(&a, &r[0], 16);
        memcpy(&b, &r[2], 16);
        nt_store16(a, &reinterpret_cast<int4 *>(dst)[0]);
        nt_store16(b, &reinterpret_cast<int4 *>(dst)[1]);
      } else if constexpr (VEC * sizeof(OUT) == 16) {
        int4 a;
        memcpy(&a, &r[0], 16);
        nt_store16(a, &reinterpret_cast<int4 *>(dst)[0]);
      } else {
        int2 a;
        memcpy(&a, &r[0], 8);
        reinterpret_cast<int2 *>(dst)[0] = a;
      }
    }
  }
  for (uint64_t i = nvec * VEC + (uint64_t)blockIdx.x * kEncBS + threadIdx.x; i < n; i += stride) {
    K key = keys[i];
    OUT r = (OUT)null_label;
    if (bit_valid(valid, i)) {
      int64_t lab = key == EMPTY ? sent : hot_lookup(key);
      if (lab < 0 && key != EMPTY && global_needed) {
        uint64_t sl = (uint64_t)slot_hash(key) & mask;
        while (true) {
          const EncSlot<K> e1 = table[sl];
          if (e1.key == key) {
            lab = (int64_t)e1.label;
            break;
          }
          if (e1.key == EMPTY) break;
          sl = (sl + 1) & mask;
        }
      }
      r = finish(key, lab);
    }
    out[i] = r;
  }
  if (count_stats) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      st_miss += __shfl_down(st_miss, off, 64);
      st_rows += __shfl_down(st_rows, off, 64);
    }
    if (lane_id() == 0) {
      atomicAdd(&g_enc_stats[0], (unsigned long long)st_miss);
      atomicAdd(&g_enc_stats[1], (unsigned long long)st_rows);
    }
  }
}

}  // namespace nvt
