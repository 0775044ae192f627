// String categoricals on the device: Arrow string buffers (offsets + chars + validity) -> the
// 64-bit surrogate keys the host path computes with pandas.util.hash_array(v, categorize=False)
// (SipHash-2-4 keyed with "0123456789123456" over the UTF-8 bytes, then pandas' mixing step),
// plus the {surrogate -> string} dictionary's device half: one representative string per
// distinct surrogate (first appearance), a byte-wise collision check, and a gather of the
// representatives into compact Arrow buffers.
//
// Chars are read with aligned 4-byte loads only: one lane hashes one string (SipHash chains its
// blocks), and every 8-byte block is assembled from three aligned words with v_alignbyte_b32.
// A lane reads no word that holds none of its string's bytes, so the chars buffer needs to be
// readable only up to the 4-byte boundary after its last byte.
#include "nvt_common.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

// ---- SipHash-2-4, pandas' key ---------------------------------------------------------------
// k0 / k1 = the key bytes "01234567" / "89123456" read little-endian (pandas/_libs/hashing.pyx)
constexpr uint64_t kSipK0 = 0x3736353433323130ull;
constexpr uint64_t kSipK1 = 0x3635343332313938ull;

// 64-bit rotate as two 32-bit funnel shifts (v_alignbit_b32 each); r in 1..31
template <int R>
__device__ __forceinline__ uint64_t rotl64(uint64_t x) {
  static_assert(R > 0 && R < 32, "rotate by 1..31");
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  const uint32_t nhi = __builtin_amdgcn_alignbit(hi, lo, 32 - R);
  const uint32_t nlo = __builtin_amdgcn_alignbit(lo, hi, 32 - R);
  return ((uint64_t)nhi << 32) | nlo;
}
// rotate by 32: swap the halves (no instruction)
__device__ __forceinline__ uint64_t swap32(uint64_t x) { return (x << 32) | (x >> 32); }

struct Sip {
  uint64_t v0, v1, v2, v3;
  __device__ __forceinline__ Sip()
      : v0(0x736f6d6570736575ull ^ kSipK0), v1(0x646f72616e646f6dull ^ kSipK1),
        v2(0x6c7967656e657261ull ^ kSipK0), v3(0x7465646279746573ull ^ kSipK1) {}
  __device__ __forceinline__ void round() {
    v0 += v1; v1 = rotl64<13>(v1); v1 ^= v0; v0 = swap32(v0);
    v2 += v3; v3 = rotl64<16>(v3); v3 ^= v2;
    v0 += v3; v3 = rotl64<21>(v3); v3 ^= v0;
    v2 += v1; v1 = rotl64<17>(v1); v1 ^= v2; v2 = swap32(v2);
  }
  __device__ __forceinline__ void block(uint64_t m) {
    v3 ^= m;
    round();
    round();
    v0 ^= m;
  }
  __device__ __forceinline__ uint64_t finish() {
    v2 ^= 0xff;
    round();
    round();
    round();
    round();
    return v0 ^ v1 ^ v2 ^ v3;
  }
};

// pandas/core/util/hashing.py, end of _hash_ndarray
__device__ __forceinline__ uint64_t pandas_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// ---- reading one string with aligned words --------------------------------------------------
// Word j is the aligned 4-byte word at (start & ~3) + 4 j; words past the last one that holds a
// byte of the string read as 0 (never loaded).
struct StrWords {
  const uint32_t *w;
  uint32_t sh;       // start & 3
  uint64_t nwords;   // words holding at least one byte of the string
  uint64_t len;
  __device__ __forceinline__ StrWords(const uint8_t *p, uint64_t len_) : len(len_) {
    sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    w = reinterpret_cast<const uint32_t *>(p - sh);  // (pointer arithmetic keeps global loads)
    nwords = len ? (sh + len + 3) >> 2 : 0;
  }
  __device__ __forceinline__ uint32_t word(uint64_t j) const { return j < nwords ? w[j] : 0u; }
  // bytes [8k, 8k + 8) of the string from the words 2k, 2k+1, 2k+2 (little-endian)
  static __device__ __forceinline__ uint64_t assemble(uint32_t a, uint32_t b, uint32_t c, uint32_t sh) {
    const uint32_t lo = __builtin_amdgcn_alignbyte(b, a, sh);
    const uint32_t hi = __builtin_amdgcn_alignbyte(c, b, sh);
    return ((uint64_t)hi << 32) | lo;
  }
  // block k with the bytes at or past `len` cleared
  __device__ __forceinline__ uint64_t block(uint64_t k) const {
    uint64_t m = assemble(word(2 * k), word(2 * k + 1), word(2 * k + 2), sh);
    const uint64_t rem = len - 8 * k;  // bytes of the string in this block (>= 1)
    if (rem < 8) m &= (1ull << (8 * rem)) - 1;
    return m;
  }
};

template <typename O>
__device__ __forceinline__ void string_at(const O *offsets, const uint8_t *chars, uint64_t i,
                                          const uint8_t **p, uint64_t *len) {
  const int64_t base = (int64_t)offsets[0];
  const int64_t b = (int64_t)offsets[i], e = (int64_t)offsets[i + 1];
  *p = chars + (b - base);
  *len = e > b ? (uint64_t)(e - b) : 0;
}

__device__ __forceinline__ uint64_t surrogate(const uint8_t *p, uint64_t len) {
  StrWords s(p, len);
  Sip h;
  const uint64_t nb = len >> 3;
  uint32_t a = s.word(0);
  for (uint64_t k = 0; k < nb; ++k) {
    const uint32_t b = s.word(2 * k + 1), c = s.word(2 * k + 2);
    h.block(StrWords::assemble(a, b, c, s.sh));
    a = c;
  }
  // last block: the 0..7 tail bytes + (len & 0xff) in the top byte
  const uint64_t tl = len & 7;
  uint64_t t = 0;
  if (tl) {
    t = StrWords::assemble(a, s.word(2 * nb + 1), s.word(2 * nb + 2), s.sh);
    t &= (1ull << (8 * tl)) - 1;
  }
  h.block(t | (len << 56));
  return pandas_mix(h.finish());
}

template <typename O>
__global__ __launch_bounds__(kBlock) void str_hash_kernel(const O *offsets, const uint8_t *chars,
                                                          const uint8_t *valid, uint64_t n,
                                                          int64_t *out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    uint64_t key = 0;
    if (bit_valid(valid, i)) {
      const uint8_t *p;
      uint64_t len;
      string_at(offsets, chars, i, &p, &len);
      key = surrogate(p, len);
    }
    out[i] = (int64_t)key;
  }
}

template <typename I>
__global__ __launch_bounds__(kBlock) void str_take_kernel(const int64_t *dict_keys, uint64_t n_dict,
                                                          const I *idx, const uint8_t *valid,
                                                          uint64_t n, int64_t *out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    int64_t key = 0;
    if (bit_valid(valid, i)) {
      const uint64_t j = (uint64_t)(int64_t)idx[i];
      if (j < n_dict) key = dict_keys[j];
    }
    out[i] = key;
  }
}

// ---- dedup + verify -------------------------------------------------------------------------
// Workspace: table keys u64[cap] | table rows u32[cap] | sentinel row u32 (+pad) |
//            flags u32[n + 1] (+pad) | scan chunk totals u64[scan_chunks(n + 1)]
// A key equal to kEmpty never enters the table: its rows share the dedicated sentinel word.
constexpr uint64_t kEmpty = 0x8000000000000000ull;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

struct DedupWs {
  uint64_t cap;
  unsigned long long *tkeys;
  uint32_t *trows;
  uint32_t *sent_row;
  uint32_t *flags;
  unsigned long long *chunk_tot;
  uint64_t bytes;
};

uint64_t dedup_capacity(uint64_t n) {
  uint64_t want = n + n / 3 + 1, cap = 64;
  while (cap < want) cap <<= 1;
  return cap;
}

inline uint64_t up256(uint64_t b) { return (b + 255) & ~255ull; }

DedupWs dedup_layout(void *ws, uint64_t n) {
  DedupWs d;
  d.cap = dedup_capacity(n);
  uint8_t *p = static_cast<uint8_t *>(ws);
  uint64_t off = 0;
  d.tkeys = reinterpret_cast<unsigned long long *>(p + off);
  off += up256(d.cap * 8);
  d.trows = reinterpret_cast<uint32_t *>(p + off);
  off += up256(d.cap * 4);
  d.sent_row = reinterpret_cast<uint32_t *>(p + off);
  off += 256;
  d.flags = reinterpret_cast<uint32_t *>(p + off);
  off += up256((n + 1) * 4);
  d.chunk_tot = reinterpret_cast<unsigned long long *>(p + off);
  off += up256(scan_chunks(n + 1) * 8);
  d.bytes = off;
  return d;
}

__device__ __forceinline__ uint64_t home_slot(uint64_t key, uint64_t mask) { return fmix64(key) & mask; }

__global__ __launch_bounds__(kBlock) void dedup_clear_kernel(unsigned long long *tkeys, uint32_t *trows,
                                                             uint64_t cap, uint32_t *sent_row,
                                                             uint64_t *out_counts) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  for (uint64_t i = t; i < cap; i += (uint64_t)gridDim.x * kBlock) {
    tkeys[i] = kEmpty;
    trows[i] = kNoRow;
  }
  if (t == 0) {
    *sent_row = kNoRow;
    out_counts[0] = 0;
    out_counts[1] = 0;
  }
}

// Claim each valid row's key (64-bit CAS into an empty slot), then keep the smallest row per key.
__global__ __launch_bounds__(kBlock) void dedup_insert_kernel(const int64_t *keys, const uint8_t *valid,
                                                              uint64_t n, unsigned long long *tkeys,
                                                              uint32_t *trows, uint64_t mask,
                                                              uint32_t *sent_row) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    if (!bit_valid(valid, i)) continue;
    const unsigned long long k = (unsigned long long)keys[i];
    uint32_t *slot_row;
    if (k == kEmpty) {
      slot_row = sent_row;
    } else {
      uint64_t h = home_slot(k, mask);
      while (true) {
        unsigned long long cur = tkeys[h];
        if (cur == kEmpty) cur = atomicCAS(&tkeys[h], kEmpty, k);
        if (cur == kEmpty || cur == k) break;
        h = (h + 1) & mask;
      }
      slot_row = &trows[h];
    }
    // rows arrive roughly in ascending order: a plain read first keeps a frequent key from
    // serialising every one of its rows on one atomic
    if (*(volatile uint32_t *)slot_row > (uint32_t)i) atomicMin(slot_row, (uint32_t)i);
  }
}

template <typename I>
__device__ __forceinline__ uint64_t str_index(const I *index, uint64_t i) {
  return index ? (uint64_t)(int64_t)index[i] : i;
}

template <typename O>
__device__ __forceinline__ void string_of(const O *offsets, const uint8_t *chars, uint64_t n_strings,
                                          uint64_t s, const uint8_t **p, uint64_t *len) {
  if (s < n_strings) {
    string_at(offsets, chars, s, p, len);
  } else {  // out-of-range index: the empty string (never dereferenced)
    *p = chars;
    *len = 0;
  }
}

// Each valid row finds its slot again: flag = row is its key's representative; otherwise its
// bytes are compared with the representative's (length, then 8-byte blocks).
template <typename O, typename I>
__global__ __launch_bounds__(kBlock) void dedup_verify_kernel(
    const int64_t *keys, const uint8_t *valid, uint64_t n, const I *index, const O *offsets,
    const uint8_t *chars, uint64_t n_strings, const unsigned long long *tkeys, const uint32_t *trows,
    uint64_t mask, const uint32_t *sent_row, uint32_t *flags, uint64_t *out_counts) {
  unsigned long long bad = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n;
       i += (uint64_t)gridDim.x * kBlock) {
    uint32_t flag = 0;
    if (i < n && bit_valid(valid, i)) {
      const unsigned long long k = (unsigned long long)keys[i];
      uint32_t rep;
      if (k == kEmpty) {
        rep = *sent_row;
      } else {
        uint64_t h = home_slot(k, mask);
        while (tkeys[h] != k) h = (h + 1) & mask;
        rep = trows[h];
      }
      if (rep == (uint32_t)i) {
        flag = 1;
      } else {
        const uint8_t *pa, *pb;
        uint64_t la, lb;
        string_of(offsets, chars, n_strings, str_index(index, i), &pa, &la);
        string_of(offsets, chars, n_strings, str_index(index, (uint64_t)rep), &pb, &lb);
        bool differ = la != lb;
        if (!differ) {
          const StrWords a(pa, la), b(pb, lb);
          const uint64_t nblk = (la + 7) >> 3;
          for (uint64_t q = 0; q < nblk && !differ; ++q) differ = a.block(q) != b.block(q);
        }
        bad += differ;
      }
    }
    flags[i] = flag;
  }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if (lane_id() == 0 && bad) atomicAdd((unsigned long long *)&out_counts[1], bad);
}

// flags now hold the exclusive prefix: row i is a representative iff flags[i + 1] != flags[i]
template <typename I>
__global__ __launch_bounds__(kBlock) void dedup_emit_kernel(const int64_t *keys, uint64_t n, const I *index,
                                                            const uint32_t *pos, int64_t *out_keys,
                                                            int64_t *out_strs, uint64_t *out_counts) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t p = pos[i];
    if (pos[i + 1] != p) {
      out_keys[p] = keys[i];
      out_strs[p] = (int64_t)str_index(index, i);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_counts[0] = pos[n];
}

// ---- gather ---------------------------------------------------------------------------------
template <typename O>
__global__ __launch_bounds__(kBlock) void gather_len_kernel(const int64_t *strs, uint64_t m,
                                                            const O *offsets, uint64_t n_strings,
                                                            uint32_t *lens) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j <= m;
       j += (uint64_t)gridDim.x * kBlock) {
    uint32_t len = 0;
    if (j < m) {
      const uint64_t s = (uint64_t)strs[j];
      if (s < n_strings) {
        const int64_t b = (int64_t)offsets[s], e = (int64_t)offsets[s + 1];
        len = e > b ? (uint32_t)(e - b) : 0;
      }
    }
    lens[j] = len;
  }
}

// 16 lanes per string: lane l copies bytes l, l + 16, ... (the destinations are packed, so any
// byte alignment occurs on both sides)
constexpr int kGatherLanes = 16;
template <typename O>
__global__ __launch_bounds__(kBlock) void gather_copy_kernel(const int64_t *strs, uint64_t m,
                                                             const O *offsets, const uint8_t *chars,
                                                             uint64_t n_strings, const uint32_t *pos,
                                                             int64_t *out_offsets, uint8_t *out_chars,
                                                             uint64_t out_capacity) {
  const uint64_t groups = (uint64_t)gridDim.x * (kBlock / kGatherLanes);
  const uint32_t sub = threadIdx.x % kGatherLanes;
  for (uint64_t j = (uint64_t)blockIdx.x * (kBlock / kGatherLanes) + threadIdx.x / kGatherLanes; j <= m;
       j += groups) {
    const uint64_t dst = pos[j];
    if (sub == 0) out_offsets[j] = (int64_t)dst;
    if (j == m) continue;
    const uint64_t end = pos[j + 1];
    if (end < dst || end > out_capacity) continue;  // repeated strings: out_offsets[m] tells it
    const uint64_t s = (uint64_t)strs[j];
    if (s >= n_strings) continue;
    const uint8_t *src = chars + ((int64_t)offsets[s] - (int64_t)offsets[0]);
    for (uint64_t b = sub; b < end - dst; b += kGatherLanes) out_chars[dst + b] = src[b];
  }
}

inline bool width_ok(int w) { return w == 4 || w == 8; }

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_str_hash(const void *offsets, int offset_bytes, const uint8_t *chars, const uint8_t *valid,
                 uint64_t n, int64_t *out, void *stream) {
  NVT_CHECK_ARG(width_ok(offset_bytes), "offset_bytes must be 4 or 8");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(offsets && chars && out, "null pointer");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(chars) & 3) == 0, "chars must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("str_hash", n * (offset_bytes + 8), s);
  const unsigned grid = stream_grid(n, kBlock);
  if (offset_bytes == 4)
    str_hash_kernel<int32_t><<<grid, kBlock, 0, s>>>((const int32_t *)offsets, chars, valid, n, out);
  else
    str_hash_kernel<int64_t><<<grid, kBlock, 0, s>>>((const int64_t *)offsets, chars, valid, n, out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_str_take_keys(const int64_t *dict_keys, uint64_t n_dict, const void *indices, int index_bytes,
                      const uint8_t *valid, uint64_t n, int64_t *out, void *stream) {
  NVT_CHECK_ARG(width_ok(index_bytes), "index_bytes must be 4 or 8");
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(indices && out && (dict_keys || n_dict == 0), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("str_take_keys", n * (index_bytes + 16), s);
  const unsigned grid = stream_grid(n, kBlock * 4);
  if (index_bytes == 4)
    str_take_kernel<int32_t><<<grid, kBlock, 0, s>>>(dict_keys, n_dict, (const int32_t *)indices, valid, n, out);
  else
    str_take_kernel<int64_t><<<grid, kBlock, 0, s>>>(dict_keys, n_dict, (const int64_t *)indices, valid, n, out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_str_dedup_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null pointer");
  NVT_CHECK_ARG(n < 0xFFFFFFFFull, "more than 2^32 - 2 rows");
  *bytes = dedup_layout(nullptr, n).bytes;
  return NVT_OK;
}

int nvt_str_dedup(const int64_t *keys, const uint8_t *valid, uint64_t n, const void *index, int index_bytes,
                  const void *offsets, int offset_bytes, const uint8_t *chars, uint64_t n_strings, void *ws,
                  uint64_t ws_bytes, int64_t *out_keys, int64_t *out_strs, uint64_t *out_counts,
                  void *stream) {
  NVT_CHECK_ARG(width_ok(offset_bytes), "offset_bytes must be 4 or 8");
  NVT_CHECK_ARG(index == nullptr || width_ok(index_bytes), "index_bytes must be 4 or 8");
  NVT_CHECK_ARG(n < 0xFFFFFFFFull, "more than 2^32 - 2 rows");
  NVT_CHECK_ARG(out_counts && ws, "null pointer");
  const DedupWs d = dedup_layout(ws, n);
  NVT_CHECK_ARG(ws_bytes >= d.bytes, "workspace smaller than nvt_str_dedup_ws_bytes");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (n) {
    NVT_CHECK_ARG(keys && out_keys && out_strs, "null pointer");
    NVT_CHECK_ARG(offsets && chars, "null string buffers");
    NVT_CHECK_ARG(n_strings > 0, "no strings");
    NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(chars) & 3) == 0, "chars must be 4-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("str_dedup", n * 40 + d.cap * 12, s);
  dedup_clear_kernel<<<stream_grid(d.cap, kBlock * 4), kBlock, 0, s>>>(d.tkeys, d.trows, d.cap,
                                                                         d.sent_row, out_counts);
  NVT_CHECK_LAUNCH();
  if (n == 0) return NVT_OK;
  const uint64_t mask = d.cap - 1;
  const unsigned grid = stream_grid(n + 1, kBlock * 2);
  dedup_insert_kernel<<<grid, kBlock, 0, s>>>(keys, valid, n, d.tkeys, d.trows, mask, d.sent_row);
  NVT_CHECK_LAUNCH();
#define NVT_STR_VERIFY(O, I)                                                                          \
  dedup_verify_kernel<O, I><<<grid, kBlock, 0, s>>>(keys, valid, n, (const I *)index, (const O *)offsets, \
                                                    chars, n_strings, d.tkeys, d.trows, mask, d.sent_row, \
                                                    d.flags, out_counts)
  if (offset_bytes == 4 && index_bytes == 8) NVT_STR_VERIFY(int32_t, int64_t);
  else if (offset_bytes == 4) NVT_STR_VERIFY(int32_t, int32_t);
  else if (index_bytes == 8) NVT_STR_VERIFY(int64_t, int64_t);
  else NVT_STR_VERIFY(int64_t, int32_t);
#undef NVT_STR_VERIFY
  NVT_CHECK_LAUNCH();
  int rc = exclusive_scan_u32(d.flags, n + 1, d.chunk_tot, s);
  if (rc != NVT_OK) return rc;
  if (index_bytes == 8)
    dedup_emit_kernel<int64_t><<<grid, kBlock, 0, s>>>(keys, n, (const int64_t *)index, d.flags, out_keys,
                                                       out_strs, out_counts);
  else
    dedup_emit_kernel<int32_t><<<grid, kBlock, 0, s>>>(keys, n, (const int32_t *)index, d.flags, out_keys,
                                                       out_strs, out_counts);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

int nvt_str_gather_ws_bytes(uint64_t m, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null pointer");
  NVT_CHECK_ARG(m < 0xFFFFFFFFull, "more than 2^32 - 2 strings");
  *bytes = up256((m + 1) * 4) + up256(scan_chunks(m + 1) * 8);
  return NVT_OK;
}

int nvt_str_gather(const int64_t *strs, uint64_t m, const void *offsets, int offset_bytes,
                   const uint8_t *chars, uint64_t n_strings, void *ws, uint64_t ws_bytes,
                   int64_t *out_offsets, uint8_t *out_chars, uint64_t out_capacity, void *stream) {
  NVT_CHECK_ARG(width_ok(offset_bytes), "offset_bytes must be 4 or 8");
  NVT_CHECK_ARG(m < 0xFFFFFFFFull, "more than 2^32 - 2 strings");
  NVT_CHECK_ARG(out_capacity < 0xFFFFFFFFull, "out_capacity must be below 4 GiB");
  NVT_CHECK_ARG(ws && out_offsets, "null pointer");
  uint64_t need = 0;
  nvt_str_gather_ws_bytes(m, &need);
  NVT_CHECK_ARG(ws_bytes >= need, "workspace smaller than nvt_str_gather_ws_bytes");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
  if (m) NVT_CHECK_ARG(strs && offsets && chars && out_chars, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("str_gather", m * 24, s);
  uint32_t *lens = static_cast<uint32_t *>(ws);
  auto *chunk_tot = reinterpret_cast<unsigned long long *>(static_cast<uint8_t *>(ws) + up256((m + 1) * 4));
  const unsigned grid = stream_grid(m + 1, kBlock * 4);
  if (offset_bytes == 4)
    gather_len_kernel<int32_t><<<grid, kBlock, 0, s>>>(strs, m, (const int32_t *)offsets, n_strings, lens);
  else
    gather_len_kernel<int64_t><<<grid, kBlock, 0, s>>>(strs, m, (const int64_t *)offsets, n_strings, lens);
  NVT_CHECK_LAUNCH();
  int rc = exclusive_scan_u32(lens, m + 1, chunk_tot, s);
  if (rc != NVT_OK) return rc;
  const unsigned cgrid = stream_grid(m + 1, kBlock / kGatherLanes * 4);
  if (offset_bytes == 4)
    gather_copy_kernel<int32_t><<<cgrid, kBlock, 0, s>>>(strs, m, (const int32_t *)offsets, chars, n_strings,
                                                         lens, out_offsets, out_chars, out_capacity);
  else
    gather_copy_kernel<int64_t><<<cgrid, kBlock, 0, s>>>(strs, m, (const int64_t *)offsets, chars, n_strings,
                                                         lens, out_offsets, out_chars, out_capacity);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
