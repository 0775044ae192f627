// Parquet in, snappy: the raw snappy bodies of PLAIN data pages inflated on the device (DESIGN.md,
// "Snappy pages in the parquet reader").  The host (nvt_pq_decode_chunk_inflate, nvt_parquet.hip) has
// walked the page headers and staged the compressed bodies as the file holds them with one record per
// page; here every page's VALUES are written into the hole the page left in the packed values.
//
//   grid     one workgroup of ONE wave per page, all pages of a partition in one launch.  A page is a
//            serial format (an element's place follows from every element before it), so a second wave
//            would only wait for the first; pages are independent and a partition has hundreds.
//   input    the compressed body passes through an LDS RING of kRing = 4096 bytes in chunks of 64
//            lanes x 16 bytes.  Ring positions are COORDINATES: the body's byte j has coordinate
//            j + (address of the body & 15), so a chunk is 64 aligned 16-byte loads; the two lanes that
//            hold the body's first and last bytes load those byte by byte (nothing outside the body is
//            read).  A chunk is loaded whenever 3072 bytes or fewer lie in front of the parse position.
//   parse    a ROUND looks at the 64 input bytes from position p on.  Lane l decodes the element that
//            WOULD start at p + l (tag kind, the literal's length bytes, span in the input) from the
//            ring; nxt[l] = l + span (64 = leaves the window).  Which lanes are real starts follows by
//            pointer jumping: six rounds of nxt = nxt[nxt] (ds_bpermute), during which lane i applies
//            the powers named by the bits of i to position 0 -- lane i ends up holding the start of the
//            round's i-th element, which is the compaction as well.  Lane i decodes that element again
//            (5 LDS bytes), an exclusive wave scan of the output lengths places it.  The element that
//            reaches past the window is the round's last one and sets the next p.
//   checks   per element, by its lane, before anything of the round is written; the first failing
//            element in stream order gives the page's status word and ends the page.
//   output   the last 64 KiB of output live in an LDS WINDOW (position & 65535).  A round's elements are
//            materialised in GROUPS: the longest prefix of the remaining elements whose sources end at
//            or before the finished position F (literals always; a copy when its source does: an
//            overlapping copy reads start - offset + (i mod offset), so its source ends at its start).
//            A group is written byte-parallel: lane t takes output byte F + t, finds its element by
//            binary search over the round's start table in LDS and gathers its byte from the ring or
//            the window.  Copies are 64 bytes at most; a literal of 64 bytes or more is the round's
//            last element and is moved by the whole wave on its own, 4 bytes per lane and step, in
//            pieces of what the ring holds.
//   flush    finished window bytes go to dst as aligned 4-byte stores, consecutive over the lanes (two
//            window words and a funnel shift per lane), whenever 2048 bytes have gathered and at the
//            end.  With NVT_INFLATE_V1_LEVELS the first 4 + L bytes stay in the window and are never
//            stored; L is read from the window once four bytes exist, nothing is stored before.
//   LDS      window 65536 + ring 4096 + two tables of 65 / 64 words = 70 148 bytes: two workgroups per
//            CU in 160 KiB, 512 pages in flight on 256 CUs.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_prof.hpp"

namespace nvt {
namespace {

constexpr uint32_t kWin = 65536, kWinMask = kWin - 1;     // output window, bytes
constexpr uint32_t kRing = 4096, kRingMask = kRing - 1;   // input ring, bytes
constexpr uint32_t kChunk = 64 * 16;                      // one refill
constexpr uint32_t kFlushAt = 2048;                       // unflushed bytes that trigger a flush
constexpr uint32_t kLit = 0x80000000u;                    // src table: a literal (ring coordinate below it)
constexpr uint32_t kMaxBytes = 0x7FFFFFFFu;               // a page's compressed / inflated size stays below
static_assert(kRing - kChunk == 3072 && kRing >= 64 + 64 + 8, "a round's literals lie inside the ring");
static_assert(kWin + kRing + 65 * 4 + 64 * 4 <= 80 * 1024, "two workgroups per CU");
static_assert(sizeof(nvt_inflate_page) == 40 && offsetof(nvt_inflate_page, dst_at) == 16 &&
                  offsetof(nvt_inflate_page, flags) == 32,
              "nvt_inflate_page: {src_at, src_bytes, dst_at, dst_bytes, flags, pad}");

struct Lds {
  uint32_t win[kWin / 4];
  uint32_t ring[kRing / 4];
  uint32_t out_at[65];   // output position of the round's element i; [count] = behind the last small one
  uint32_t src[64];      // kLit | ring coordinate of a literal's bytes, else the copy's offset
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// bytes [c, c + 4) of a ring of words (mask in bytes), c at any alignment
__device__ __forceinline__ uint32_t word_at(const uint32_t *words, uint32_t c, uint32_t mask) {
  const uint32_t w0 = words[(c & mask) >> 2], w1 = words[((c + 4) & mask) >> 2];
  return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * (c & 3)));
}

struct Element {
  uint32_t hdr, len, off, span;   // tag + length / offset bytes; output bytes; copy offset; input bytes
  bool lit;
};

// the element that starts at ring coordinate c (its up to 5 header bytes are in the ring, or behind
// the body's end, where the caller's bounds decide)
__device__ __forceinline__ Element parse_at(const uint8_t *ring, uint32_t c) {
  const uint32_t b0 = ring[c & kRingMask];
  uint32_t x = 0;   // the four bytes behind the tag, little endian
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) x |= (uint32_t)ring[(c + 1 + i) & kRingMask] << (8 * i);
  Element e;
  const uint32_t kind = b0 & 3, hi = b0 >> 2;
  e.lit = kind == 0;
  e.off = 0;
  if (kind == 0) {
    const uint32_t k = hi < 60 ? 0 : hi - 59;   // length bytes
    const uint32_t m = k == 0 ? hi : (k == 4 ? x : (x & ((1u << (8 * k)) - 1u)));
    e.hdr = 1 + k;
    e.len = m >= kMaxBytes ? kMaxBytes : m + 1;   // (clamped: such a literal fails its bounds)
    e.span = e.hdr + e.len;
  } else if (kind == 1) {
    e.hdr = 2;
    e.len = 4 + (hi & 7);
    e.off = ((b0 >> 5) << 8) | (x & 0xFF);
    e.span = 2;
  } else {
    e.hdr = kind == 2 ? 3 : 5;
    e.len = hi + 1;
    e.off = kind == 2 ? (x & 0xFFFF) : x;
    e.span = e.hdr;
  }
  return e;
}

// everything one page's wave carries: uniform over the lanes
struct Page {
  const uint8_t *base;   // the body's address rounded down to 16 bytes: coordinate 0
  uint8_t *dst;          // where window position `drop` goes
  uint32_t a0, cend;     // coordinates of the body's first byte and behind its last
  uint32_t rend;         // coordinates below this are in the ring (a multiple of kChunk)
  uint32_t total, dst_bytes;
  uint32_t o, fl;        // output bytes produced / window position flushed up to
  uint32_t drop;         // window bytes in front of the values (0, or 4 + L)
  bool drop_known;
};

// loads chunks while 3072 bytes or fewer lie between coordinate c (the oldest one still needed) and
// the ring's end
__device__ __forceinline__ void refill(Lds &l, Page &pg, uint32_t c, uint32_t lane) {
  bool any = false;
  // (rend <= c: the first chunk of a body that is not 16-byte aligned, whose coordinates start at a0 > 0)
  while (pg.rend < pg.cend && (pg.rend <= c || pg.rend - c <= kRing - kChunk)) {
    const uint32_t x = pg.rend + lane * 16;
    if (x >= pg.a0 && x + 16 <= pg.cend) {
      const uint4 v = *reinterpret_cast<const uint4 *>(pg.base + x);
      uint32_t *r = &l.ring[(x & kRingMask) >> 2];
      r[0] = v.x;
      r[1] = v.y;
      r[2] = v.z;
      r[3] = v.w;
    } else if (x + 16 > pg.a0 && x < pg.cend) {   // the body's first or last bytes
      uint8_t *r = reinterpret_cast<uint8_t *>(l.ring);
      for (uint32_t b = 0; b < 16; ++b)
        if (x + b >= pg.a0 && x + b < pg.cend) r[(x + b) & kRingMask] = pg.base[x + b];
    }
    pg.rend += kChunk;
    any = true;
  }
  if (any) __syncthreads();
}

// window bytes [fl, o) -> dst, whole aligned words only unless `last`.  -> 0 or NVT_INFLATE_LENGTH
__device__ __forceinline__ uint32_t flush(Lds &l, Page &pg, bool last, uint32_t lane) {
  const uint8_t *win = reinterpret_cast<const uint8_t *>(l.win);
  if (!pg.drop_known) {
    if (pg.o < 4) return last ? NVT_INFLATE_LENGTH : 0;
    const uint64_t drop = 4ull + l.win[0];   // u32 L | L level bytes
    if (drop > pg.total || pg.total - drop != pg.dst_bytes) return NVT_INFLATE_LENGTH;
    pg.drop = (uint32_t)drop;
    pg.drop_known = true;
  }
  if (pg.fl < pg.drop) pg.fl = pg.o < pg.drop ? pg.o : pg.drop;
  if (pg.o <= pg.fl) return 0;
  uint32_t q = pg.fl;
  uint8_t *d = pg.dst + (q - pg.drop);   // window position q + i goes to d[i]; behind it o - q <= dst_bytes bytes
  uint32_t head = (4 - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 3)) & 3;
  if (head > pg.o - q) head = pg.o - q;
  if (lane < head) d[lane] = win[(q + lane) & kWinMask];
  q += head;
  d += head;
  const uint32_t nwords = (pg.o - q) >> 2;
  for (uint32_t k = lane; k < nwords; k += 64)
    *reinterpret_cast<uint32_t *>(d + 4 * k) = word_at(l.win, q + 4 * k, kWinMask);
  q += 4 * nwords;
  d += 4 * nwords;
  if (last) {
    if (lane < pg.o - q) d[lane] = win[(q + lane) & kWinMask];
    q = pg.o;
  }
  pg.fl = q;
  return 0;
}

// `n` literal bytes from ring coordinate c to window position o, all in the ring
__device__ __forceinline__ void literal_to_window(Lds &l, uint32_t c, uint32_t o, uint32_t n, uint32_t lane) {
  uint8_t *win = reinterpret_cast<uint8_t *>(l.win);
  const uint8_t *ring = reinterpret_cast<const uint8_t *>(l.ring);
  uint32_t head = (4 - (o & 3)) & 3;
  if (head > n) head = n;
  if (lane < head) win[(o + lane) & kWinMask] = ring[(c + lane) & kRingMask];
  const uint32_t nwords = (n - head) >> 2;
  for (uint32_t k = lane; k < nwords; k += 64)
    l.win[((o + head + 4 * k) & kWinMask) >> 2] = word_at(l.ring, c + head + 4 * k, kRingMask);
  const uint32_t done = head + 4 * nwords;
  if (lane < n - done) win[(o + done + lane) & kWinMask] = ring[(c + done + lane) & kRingMask];
}

// -> the page's status word
__device__ uint32_t inflate_page(Lds &l, const uint8_t *src, uint8_t *dst, const nvt_inflate_page &pd, uint32_t lane) {
  uint8_t *win = reinterpret_cast<uint8_t *>(l.win);
  const uint8_t *ring = reinterpret_cast<const uint8_t *>(l.ring);
  if (pd.src_bytes == 0) return NVT_INFLATE_TRUNCATED;
  if (pd.src_bytes >= kMaxBytes - 16 || pd.dst_bytes >= kMaxBytes) return NVT_INFLATE_LENGTH;
  Page pg;
  const uint8_t *body = src + pd.src_at;
  pg.a0 = (uint32_t)(reinterpret_cast<uintptr_t>(body) & 15);
  pg.base = body - pg.a0;
  pg.cend = pg.a0 + (uint32_t)pd.src_bytes;
  pg.rend = 0;
  pg.dst = dst + pd.dst_at;
  pg.dst_bytes = (uint32_t)pd.dst_bytes;
  pg.o = pg.fl = pg.drop = 0;
  pg.drop_known = !(pd.flags & NVT_INFLATE_V1_LEVELS);
  uint32_t c = pg.a0;   // the parse position, a coordinate
  refill(l, pg, c, lane);
  // varint(inflated length): 5 bytes at most for a length below 2^31
  uint64_t total = 0;
  for (uint32_t i = 0;; ++i) {
    if (c >= pg.cend) return NVT_INFLATE_TRUNCATED;
    if (i == 5) return NVT_INFLATE_LENGTH;
    const uint32_t b = ring[c++ & kRingMask];
    total |= (uint64_t)(b & 0x7F) << (7 * i);
    if (!(b & 0x80)) break;
  }
  if (total >= kMaxBytes) return NVT_INFLATE_LENGTH;
  pg.total = (uint32_t)total;
  if (pg.drop_known && pg.total != pg.dst_bytes) return NVT_INFLATE_LENGTH;

  while (c < pg.cend) {
    refill(l, pg, c, lane);
    // ---- which of the 64 positions start an element ----
    uint32_t nxt = 64;
    if (c + lane < pg.cend) {
      const Element e = parse_at(ring, c + lane);
      // (64 as well when the element ends the body: no element starts behind it)
      nxt = (e.span >= 64 - lane || e.span >= pg.cend - (c + lane)) ? 64 : lane + e.span;
    }
    uint32_t at = 0;   // lane i: the lane where element i of the round starts (64: there is none)
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
      const uint32_t hop = __shfl(nxt, at & 63, 64);
      if (((lane >> k) & 1) && at < 64) at = hop;
      const uint32_t two = __shfl(nxt, nxt & 63, 64);
      nxt = nxt < 64 ? two : 64;
    }
    const bool mine = at < 64;
    const uint32_t count = uni((uint32_t)__popcll(__ballot(mine)));   // >= 1: lane 0 starts one
    Element e = {0, 0, 0, 0, false};
    if (mine) e = parse_at(ring, c + at);
    // ---- exclusive scan of the output lengths: where element i goes ----
    uint32_t incl = e.len;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const uint32_t out_at = pg.o + incl - e.len;
    // ---- checks, by element; the first failing one in stream order decides ----
    uint32_t err = 0;
    if (mine) {
      const uint32_t left = pg.cend - (c + at);   // input bytes from the tag on
      if (e.hdr > left || (e.lit && e.span > left)) err = NVT_INFLATE_TRUNCATED;
      else if (!e.lit && (e.off == 0 || e.off > out_at)) err = NVT_INFLATE_OFFSET;
      else if (!e.lit && e.off > kWin) err = NVT_INFLATE_FAR;
      else if (e.len > pg.total - out_at) err = NVT_INFLATE_LENGTH;   // (out_at <= total: the elements before passed)
    }
    const uint64_t failed = __ballot(err != 0);
    if (failed) return uni(__shfl(err, (int)__builtin_ctzll(failed), 64));
    // ---- the round's tables ----
    const bool big = uni(__shfl((uint32_t)(e.lit && e.len >= 64), (int)(count - 1), 64)) != 0;
    const uint32_t nsmall = big ? count - 1 : count;
    const uint32_t small_end = big ? uni(__shfl(out_at, (int)(count - 1), 64)) : uni(__shfl(out_at + e.len, (int)(count - 1), 64));
    if (mine) {
      l.out_at[lane] = out_at;
      l.src[lane] = e.lit ? (kLit | (c + at + e.hdr)) : e.off;
    }
    if (lane == nsmall) l.out_at[lane] = small_end;
    if (lane == 63 && nsmall == 64) l.out_at[64] = small_end;
    __syncthreads();
    // ---- groups of elements whose sources are finished ----
    const uint32_t src_end = e.lit ? 0 : out_at - e.off + (e.len < e.off ? e.len : e.off);
    uint32_t g0 = 0, fin = pg.o;
    while (g0 < nsmall) {
      const uint64_t waits = __ballot(lane >= g0 && lane < nsmall && src_end > fin);
      const uint32_t g1 = waits ? (uint32_t)__builtin_ctzll(waits) : nsmall;   // > g0: element g0's source ends at or before fin
      const uint32_t gend = uni(l.out_at[g1]);
      for (uint32_t step = fin; step < gend; step += 64) {   // (uniform trip count)
        const uint32_t q = step + lane;
        const bool on = q < gend;
        uint8_t v = 0;
        if (on) {
          uint32_t lo = g0, hi = g1;
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (l.out_at[mid] <= q) lo = mid; else hi = mid;
          }
          const uint32_t first = l.out_at[lo], s = l.src[lo], d = q - first;
          if (s & kLit) {
            v = ring[((s & ~kLit) + d) & kRingMask];
          } else {
            const uint32_t dd = d < s ? d : d % s;   // an overlapping copy repeats its `s` source bytes
            v = win[(first - s + dd) & kWinMask];
          }
        }
        // every lane has gathered before any lane stores: with offsets of 65535 and 65536 a lane's
        // source is the slot that this step overwrites (a neighbour's, or its own)
        __syncthreads();
        if (on) win[q & kWinMask] = v;
      }
      __syncthreads();
      fin = gend;
      g0 = g1;
    }
    pg.o = small_end;
    const uint32_t last_at = uni(__shfl(at, (int)(count - 1), 64)), last_span = uni(__shfl(e.span, (int)(count - 1), 64));
    if (big) {   // the whole wave, in pieces of what the ring holds, flushing as it goes
      const uint32_t hdr = uni(__shfl(e.hdr, (int)(count - 1), 64));
      uint32_t left = uni(__shfl(e.len, (int)(count - 1), 64));
      uint32_t lc = c + last_at + hdr;
      while (left) {
        refill(l, pg, lc, lane);
        const uint32_t have = (pg.rend < pg.cend ? pg.rend : pg.cend) - lc;   // > 0: the literal ends inside the body
        const uint32_t take = left < have ? left : have;
        literal_to_window(l, lc, pg.o, take, lane);
        __syncthreads();
        pg.o += take;
        lc += take;
        left -= take;
        const uint32_t rc = flush(l, pg, false, lane);
        if (rc) return rc;
      }
    } else if (pg.o - pg.fl >= kFlushAt) {
      const uint32_t rc = flush(l, pg, false, lane);
      if (rc) return rc;
    }
    c += last_at + last_span;
  }
  if (pg.o != pg.total) return NVT_INFLATE_LENGTH;
  return flush(l, pg, true, lane);
}

__global__ __launch_bounds__(64) void snappy_inflate_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                            const nvt_inflate_page *__restrict__ pages,
                                                            uint32_t *__restrict__ status) {
  __shared__ Lds l;
  const nvt_inflate_page pd = pages[blockIdx.x];
  const uint32_t rc = inflate_page(l, src, dst, pd, lane_id());
  if (lane_id() == 0) status[blockIdx.x] = rc;
}

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_snappy_inflate_pages(const uint8_t *src, uint8_t *dst, const nvt_inflate_page *pages, uint64_t npages,
                             uint32_t *status, void *stream) {
  if (npages == 0) return NVT_OK;
  NVT_CHECK_ARG(src && dst && pages && status, "null pointer");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(pages) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                "tables must be aligned to their words");
  NVT_CHECK_ARG(npages < (1ull << 31), "fewer than 2^31 pages");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("snappy_inflate", npages * 8, s);
  snappy_inflate_kernel<<<(unsigned)npages, 64, 0, s>>>(src, dst, pages, status);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
