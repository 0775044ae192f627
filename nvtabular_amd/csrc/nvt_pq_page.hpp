// Parquet in, host side: the page headers, the level decoders and the ONE walk over the pages of a
// column chunk that every nvt_pq_decode_* entry point goes through (nvt_parquet.hip,
// nvt_parquet_str_in.hip).  Host code only.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"

namespace nvt {

// ---- thrift compact protocol, reading side (parquet-format's PageHeader) ----------------------
struct TReader {
  const uint8_t *p, *end;
  bool ok = true;
  uint64_t varint() {
    uint64_t v = 0;
    int sh = 0;
    while (p < end) {
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7F) << sh;
      if (!(b & 0x80)) return v;
      sh += 7;
      if (sh > 63) break;
    }
    ok = false;
    return 0;
  }
  int64_t zigzag() {
    const uint64_t v = varint();
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
  void skip_bytes(uint64_t n) {
    if ((uint64_t)(end - p) < n) {
      ok = false;
      p = end;
    } else {
      p += n;
    }
  }
  // compact types: 1 / 2 bool, 3 byte, 4 i16, 5 i32, 6 i64, 7 double, 8 binary, 9 list, 10 set,
  // 11 map, 12 struct
  void skip(int type, int depth = 0) {
    if (!ok || depth > 16) {
      ok = false;
      return;
    }
    switch (type) {
      case 1: case 2: break;
      case 3: skip_bytes(1); break;
      case 4: case 5: case 6: (void)varint(); break;
      case 7: skip_bytes(8); break;
      case 8: skip_bytes(varint()); break;
      case 9: case 10: {
        if (p >= end) { ok = false; return; }
        const uint8_t h = *p++;
        uint64_t n = h >> 4;
        if (n == 15) n = varint();
        const int et = h & 0x0F;
        for (uint64_t i = 0; i < n && ok; ++i) skip(et, depth + 1);
        break;
      }
      case 11: {
        const uint64_t n = varint();
        if (n == 0) break;
        if (p >= end) { ok = false; return; }
        const uint8_t kv = *p++;
        for (uint64_t i = 0; i < n && ok; ++i) {
          skip(kv >> 4, depth + 1);
          skip(kv & 0x0F, depth + 1);
        }
        break;
      }
      case 12: skip_struct(depth + 1); break;
      default: ok = false;
    }
  }
  // next field header of a struct: false at the stop byte
  bool field(int &fid, int &type) {
    if (p >= end) {
      ok = false;
      return false;
    }
    const uint8_t h = *p++;
    if (h == 0) return false;
    const int d = h >> 4;
    type = h & 0x0F;
    if (d == 0) fid = (int)zigzag(); else fid += d;
    return ok;
  }
  void skip_struct(int depth = 0) {
    int fid = 0, type = 0;
    while (ok && field(fid, type)) skip(type, depth);
  }
};

struct PageHead {
  int type = -1;            // 0 data page, 2 dictionary page, 3 data page v2
  int64_t uncompressed = 0, compressed = 0;
  int64_t num_values = 0;   // rows of the page (flat columns)
  int encoding = -1, def_encoding = -1, rep_encoding = -1;
  int64_t stat_nulls = -1;  // v1: DataPageHeader.statistics.null_count, -1 when the header has none
  // v2
  int64_t num_nulls = -1, def_bytes = 0, rep_bytes = 0;
  bool v2_compressed = false;
  // dictionary page
  int64_t dict_values = 0;
  int dict_encoding = -1;
};

inline bool read_page_header(TReader &r, PageHead &h) {
  int fid = 0, type = 0;
  while (r.field(fid, type)) {
    if (fid == 1 && type == 5) h.type = (int)r.zigzag();
    else if (fid == 2 && type == 5) h.uncompressed = r.zigzag();
    else if (fid == 3 && type == 5) h.compressed = r.zigzag();
    else if (fid == 5 && type == 12) {  // DataPageHeader
      int f2 = 0, t2 = 0;
      while (r.field(f2, t2)) {
        if (f2 == 1 && t2 == 5) h.num_values = r.zigzag();
        else if (f2 == 2 && t2 == 5) h.encoding = (int)r.zigzag();
        else if (f2 == 3 && t2 == 5) h.def_encoding = (int)r.zigzag();
        else if (f2 == 4 && t2 == 5) h.rep_encoding = (int)r.zigzag();
        else if (f2 == 5 && t2 == 12) {  // Statistics
          int f3 = 0, t3 = 0;
          while (r.field(f3, t3)) {
            if (f3 == 3 && t3 == 6) h.stat_nulls = r.zigzag(); else r.skip(t3);
          }
        } else r.skip(t2);
      }
    } else if (fid == 7 && type == 12) {  // DictionaryPageHeader
      int f2 = 0, t2 = 0;
      while (r.field(f2, t2)) {
        if (f2 == 1 && t2 == 5) h.dict_values = r.zigzag();
        else if (f2 == 2 && t2 == 5) h.dict_encoding = (int)r.zigzag();
        else r.skip(t2);
      }
    } else if (fid == 8 && type == 12) {  // DataPageHeaderV2
      int f2 = 0, t2 = 0;
      h.v2_compressed = true;  // the field's default
      while (r.field(f2, t2)) {
        if (f2 == 1 && t2 == 5) h.num_values = r.zigzag();
        else if (f2 == 2 && t2 == 5) h.num_nulls = r.zigzag();
        else if (f2 == 4 && t2 == 5) h.encoding = (int)r.zigzag();
        else if (f2 == 5 && t2 == 5) h.def_bytes = r.zigzag();
        else if (f2 == 6 && t2 == 5) h.rep_bytes = r.zigzag();
        else if (f2 == 7 && (t2 == 1 || t2 == 2)) h.v2_compressed = (t2 == 1);
        else r.skip(t2);
      }
    } else {
      r.skip(type);
    }
  }
  return r.ok;
}

// ---- validity bitmap writing (LSB first) -----------------------------------------------------
inline void bits_fill(uint8_t *bm, uint64_t pos, uint64_t count, bool one) {
  while (count && (pos & 7)) {  // head
    if (one) bm[pos >> 3] |= (uint8_t)(1u << (pos & 7)); else bm[pos >> 3] &= (uint8_t)~(1u << (pos & 7));
    ++pos;
    --count;
  }
  const uint64_t nbytes = count >> 3;
  if (nbytes) memset(bm + (pos >> 3), one ? 0xFF : 0x00, nbytes);
  pos += nbytes << 3;
  count -= nbytes << 3;
  while (count) {  // tail
    if (one) bm[pos >> 3] |= (uint8_t)(1u << (pos & 7)); else bm[pos >> 3] &= (uint8_t)~(1u << (pos & 7));
    ++pos;
    --count;
  }
}

// copies `count` bits of src (from its bit 0) to bm at bit `pos`; -> number of one bits copied
inline uint64_t bits_copy(uint8_t *bm, uint64_t pos, const uint8_t *src, uint64_t count) {
  uint64_t ones = 0;
  const unsigned sh = (unsigned)(pos & 7);
  const uint64_t full = count >> 3;
  uint8_t *dst = bm + (pos >> 3);
  if (sh == 0) {
    memcpy(dst, src, full);
    for (uint64_t i = 0; i < full; ++i) ones += (uint64_t)__builtin_popcount(src[i]);
    dst += full;
  } else {
    for (uint64_t i = 0; i < full; ++i) {
      const uint8_t b = src[i];
      ones += (uint64_t)__builtin_popcount(b);
      dst[0] = (uint8_t)((dst[0] & ((1u << sh) - 1u)) | (uint8_t)(b << sh));
      dst[1] = (uint8_t)(b >> (8 - sh));
      ++dst;
    }
  }
  const unsigned rem = (unsigned)(count & 7);
  if (rem) {
    const uint8_t b = (uint8_t)(src[full] & ((1u << rem) - 1u));
    ones += (uint64_t)__builtin_popcount(b);
    uint64_t q = pos + (full << 3);
    for (unsigned j = 0; j < rem; ++j, ++q) {
      if ((b >> j) & 1) bm[q >> 3] |= (uint8_t)(1u << (q & 7)); else bm[q >> 3] &= (uint8_t)~(1u << (q & 7));
    }
  }
  return ones;
}

// definition levels of one page (max level 1, RLE / bit-packed hybrid, bit width 1) -> bits
// [pos, pos + rows) of the bitmap; *valid = rows with level 1
inline bool decode_levels(const uint8_t *lv, uint64_t nbytes, uint64_t rows, uint8_t *bm, uint64_t pos,
                          uint64_t *valid) {
  TReader r{lv, lv + nbytes};
  uint64_t done = 0, ones = 0;
  while (done < rows) {
    const uint64_t head = r.varint();
    if (!r.ok) return false;
    if (head & 1) {  // bit-packed run: (head >> 1) groups of 8 levels, one bit each
      const uint64_t groups = head >> 1, nb = groups;
      if ((uint64_t)(r.end - r.p) < nb) return false;
      uint64_t take = groups * 8;
      if (take > rows - done) take = rows - done;  // (the last group is padded)
      ones += bits_copy(bm, pos + done, r.p, take);
      r.p += nb;
      done += take;
    } else {  // RLE run: (head >> 1) times the value in the next byte (bit width 1 -> 1 byte)
      uint64_t count = head >> 1;
      if (r.p >= r.end || count == 0) return false;
      const uint8_t v = *r.p++;
      if (v > 1) return false;
      if (count > rows - done) count = rows - done;
      bits_fill(bm, pos + done, count, v == 1);
      ones += v ? count : 0;
      done += count;
    }
  }
  *valid = ones;
  return true;
}

// ---- level streams of list columns ------------------------------------------------------------
// The staging streams hold one level per slot at `bw` bits (1 or 2), LSB first, continuous over the
// pages, chunks and row groups of a partition: a page's levels land at an arbitrary bit position.
// They are written 64 bits at a time through the words that hold them (memcpy: no alignment is
// asked of the buffer, which is ceil(bits / 64) words long).
inline void put_bits(uint8_t *dst, uint64_t bitpos, uint64_t v, unsigned n) {  // n in 1 .. 64, v < 2^n
  uint8_t *at = dst + (bitpos >> 6) * 8;
  const unsigned sh = (unsigned)(bitpos & 63);
  const uint64_t mask = n == 64 ? ~0ull : ((1ull << n) - 1ull);
  uint64_t w;
  memcpy(&w, at, 8);
  w = (w & ~(mask << sh)) | (v << sh);
  memcpy(at, &w, 8);
  if (sh + n > 64) {
    const uint64_t m2 = (1ull << (sh + n - 64)) - 1ull;
    memcpy(&w, at + 8, 8);
    w = (w & ~m2) | (v >> (64 - sh));
    memcpy(at + 8, &w, 8);
  }
}

// levels per value in `nbits` bits of w (its other bits 0): hist[v] += count
inline void hist_add(uint64_t w, unsigned nbits, unsigned bw, uint64_t hist[4]) {
  if (bw == 1) {
    const uint64_t ones = (uint64_t)__builtin_popcountll(w);
    hist[1] += ones;
    hist[0] += nbits - ones;
  } else {
    const uint64_t lo = w & 0x5555555555555555ull, hi = (w >> 1) & 0x5555555555555555ull;
    const uint64_t c3 = (uint64_t)__builtin_popcountll(lo & hi);
    const uint64_t c1 = (uint64_t)__builtin_popcountll(lo) - c3, c2 = (uint64_t)__builtin_popcountll(hi) - c3;
    hist[1] += c1;
    hist[2] += c2;
    hist[3] += c3;
    hist[0] += nbits / 2 - c1 - c2 - c3;
  }
}

// `nbits` bits of src (from its bit 0; ceil(nbits / 8) bytes readable) -> dst at bit `pos`, counted
inline void bits_copy_count(uint8_t *dst, uint64_t pos, const uint8_t *src, uint64_t nbits, unsigned bw,
                            uint64_t hist[4]) {
  uint64_t done = 0;
  for (; done + 64 <= nbits; done += 64) {
    uint64_t w;
    memcpy(&w, src + (done >> 3), 8);
    hist_add(w, 64, bw, hist);
    put_bits(dst, pos + done, w, 64);
  }
  if (done < nbits) {
    const unsigned rem = (unsigned)(nbits - done);
    uint64_t w = 0;
    memcpy(&w, src + (done >> 3), (rem + 7) / 8);
    w &= (1ull << rem) - 1ull;
    hist_add(w, rem, bw, hist);
    put_bits(dst, pos + done, w, rem);
  }
}

inline void bits_fill_value(uint8_t *dst, uint64_t pos, uint64_t nbits, unsigned bw, unsigned v) {
  const uint64_t pat = bw == 1 ? (v ? ~0ull : 0ull) : (uint64_t)v * 0x5555555555555555ull;
  uint64_t done = 0;
  for (; done + 64 <= nbits; done += 64) put_bits(dst, pos + done, pat, 64);  // (64 is a multiple of bw)
  if (done < nbits) put_bits(dst, pos + done, pat & ((1ull << (nbits - done)) - 1ull), (unsigned)(nbits - done));
}

// One level stream of a page (RLE / bit-packed hybrid at bit width `bw`, nbytes long, n levels) ->
// slots [slot, slot + n) of `out`; hist[v] += levels of value v.  A bit-packed run is a shifting bit
// copy (the padding of its last group is not copied), an RLE run a fill.
// -> 0, or 1: a run leaves the stream's bytes, 2: a level above max_level
inline int decode_levels_wide(const uint8_t *lv, uint64_t nbytes, uint64_t n, unsigned bw, unsigned max_level,
                              uint8_t *out, uint64_t slot, uint64_t hist[4]) {
  TReader r{lv, lv + nbytes};
  uint64_t done = 0;
  uint64_t h[4] = {0, 0, 0, 0};
  while (done < n) {
    const uint64_t head = r.varint();
    if (!r.ok) return 1;
    if (head & 1) {
      const uint64_t groups = head >> 1;
      if (groups == 0 || groups > (1ull << 40)) return 1;
      uint64_t take = groups * 8;
      if (take > n - done) take = n - done;
      const uint64_t avail = (uint64_t)(r.end - r.p);
      if (avail < groups * bw && avail * 8 < take * bw) return 1;   // (a writer may cut the last group's padding)
      bits_copy_count(out, (slot + done) * bw, r.p, take * bw, bw, h);
      r.skip_bytes(groups * bw < avail ? groups * bw : avail);
      done += take;
    } else {
      uint64_t count = head >> 1;
      if (count == 0 || r.p >= r.end) return 1;
      const unsigned v = *r.p++;
      if (v > max_level) return 2;
      if (count > n - done) count = n - done;
      bits_fill_value(out, (slot + done) * bw, count * bw, bw, v);
      h[v] += count;
      done += count;
    }
  }
  for (unsigned v = max_level + 1; v < 4; ++v)
    if (h[v]) return 2;
  for (int v = 0; v < 4; ++v) hist[v] += h[v];
  return 0;
}

// snappy, raw block format (nvt_parquet.hip) -> uncompressed bytes written, or -1 on malformed input /
// a block that does not fit `cap`
int64_t snappy_uncompress(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap);

// ---- the page walk ------------------------------------------------------------------------------
// What an entry point states about its chunk.  `who` is the entry point's name: the prefix of every
// error message.  `expect_rows` counts what a page header's num_values counts: rows of a flat
// column, SLOTS of a list column.  scratch: room for the chunk's dictionary + its largest page
// uncompressed (include/nvt_hip.h); may be null for an uncompressed chunk.
struct PageWalk {
  const char *who;
  const uint8_t *chunk;
  uint64_t chunk_bytes;
  int codec;   // parquet CompressionCodec: 0 UNCOMPRESSED, 1 SNAPPY
  uint64_t expect_rows;
  uint8_t *scratch;
  uint64_t scratch_bytes;
};

// `nsrc` bytes of a page -> its `want` uncompressed bytes: the bytes themselves, or scratch from `at` on
inline int page_bytes(const PageWalk &w, const uint8_t *src, uint64_t nsrc, uint64_t want, bool compressed,
                      uint64_t at, const uint8_t **out) {
  if (!compressed) {
    if (nsrc != want) {
      set_error("%s: an uncompressed page of %llu bytes that says %llu", w.who, (unsigned long long)nsrc,
                (unsigned long long)want);
      return NVT_EINVAL;
    }
    *out = src;
    return NVT_OK;
  }
  if (w.scratch == nullptr || w.scratch_bytes < at || w.scratch_bytes - at < want) {
    set_error("%s: scratch too small for a page of %llu bytes", w.who, (unsigned long long)want);
    return NVT_EINVAL;
  }
  if (snappy_uncompress(src, nsrc, w.scratch + at, want) != (int64_t)want) {
    set_error("%s: malformed snappy block", w.who);
    return NVT_EINVAL;
  }
  *out = w.scratch + at;
  return NVT_OK;
}

// The level sink of a flat column: definition levels at max level 0 (none) or 1 -> the validity
// bitmap from bit `bit0` on.  (The list sink, with repetition levels, is in nvt_parquet.hip.)
//
// A level sink has: kNested (repetition levels allowed), has(s) (stream s -- 0 repetition, 1
// definition -- is in a v1 body and is decoded), v1_encodings, stream (one level stream of a page,
// *pvalid = the page's non-null values once the definition levels are known), all_valid (a page whose
// levels are not looked at) and close.
struct FlatLevels {
  static constexpr bool kNested = false;
  uint8_t *valid;
  uint64_t bit0;
  int max_def;
  // what is wrong with the caller's arguments, or null
  const char *bad_args() const {
    if (max_def != 0 && max_def != 1) return "flat columns: max definition level 0 / 1";
    return max_def == 0 || valid ? nullptr : "null validity buffer";
  }
  bool has(int s) const { return s == 1 && max_def == 1; }
  int v1_encodings(const char *who, const PageHead &h) const {
    if (max_def == 0 || h.def_encoding == 3) return NVT_OK;  // RLE (the hybrid)
    set_error("%s: definition level encoding %d", who, h.def_encoding);
    return NVT_EUNSUPPORTED;
  }
  int stream(const char *who, int, const uint8_t *lv, uint64_t nbytes, uint64_t row0, uint64_t prow,
             uint64_t *pvalid) {
    if (decode_levels(lv, nbytes, prow, valid, bit0 + row0, pvalid)) return NVT_OK;
    set_error("%s: malformed definition levels", who);
    return NVT_EINVAL;
  }
  void all_valid(uint64_t row0, uint64_t prow) {
    if (max_def == 1) bits_fill(valid, bit0 + row0, prow, true);
  }
  int close(const char *) { return NVT_OK; }
};

// What a value sink that neither takes a dictionary page nor keeps pages compressed answers.
//
// A value sink has: kKeepsDictionary (the dictionary stays at the bottom of the scratch and pages are
// inflated behind it, 16-byte aligned; otherwise every page is inflated at offset 0),
// takes_dictionary / dictionary (the dictionary page: asked before it is inflated, handed over
// after), accepts (the page's value encoding, asked before anything is inflated), stays_compressed /
// compressed_page (a snappy body that is handed over as it is, its rows all valid) and page (`pvalid`
// values in [q, pend) of a page with this header).
struct ValueSink {
  static constexpr bool kKeepsDictionary = false;
  bool takes_dictionary(const PageHead &) const { return false; }
  int dictionary(const char *, const PageHead &, const uint8_t *) { return NVT_EINVAL; }
  bool stays_compressed(const PageHead &, uint64_t, uint64_t) const { return false; }
  int compressed_page(const char *, const PageHead &, const uint8_t *, uint64_t, uint64_t) { return NVT_EINVAL; }
};

inline bool by_dictionary(const PageHead &h) { return h.encoding == 2 || h.encoding == 8; }   // PLAIN_ / RLE_DICTIONARY

// accepts() of the sinks that take PLAIN values and dictionary indices
inline int plain_or_dictionary(const char *who, const PageHead &h, bool have_dict) {
  if (h.encoding != 0 && !by_dictionary(h)) {
    set_error("%s: value encoding %d (PLAIN and dictionary indices are decoded here)", who, h.encoding);
    return NVT_EUNSUPPORTED;
  }
  if (by_dictionary(h) && !have_dict) {
    set_error("%s: dictionary indices without a dictionary page", who);
    return NVT_EINVAL;
  }
  return NVT_OK;
}

// Walks the pages of a column chunk until they hold w.expect_rows rows: header, bounds, codec, the
// split of a v1 / v2 body into levels and values, row accounting.  The levels go to `lv`, the
// dictionary page and the values to `vs`; what they refuse ends the walk with their return code.
template <typename Levels, typename Values>
int walk_pages(const PageWalk &w, Levels &lv, Values &vs) {
  if (w.codec != 0 && w.codec != 1) {
    set_error("%s: codec %d (UNCOMPRESSED and SNAPPY are decoded here)", w.who, w.codec);
    return NVT_EUNSUPPORTED;
  }
  const uint8_t *p = w.chunk, *end = w.chunk + w.chunk_bytes;
  uint64_t rows = 0;
  bool have_dict = false;
  uint64_t scratch_at = 0;   // scratch below this offset holds the dictionary
  int rc;
  while (p < end && rows < w.expect_rows) {
    TReader r{p, end};
    PageHead h;
    if (!read_page_header(r, h)) {
      set_error("%s: malformed page header at byte %llu", w.who, (unsigned long long)(p - w.chunk));
      return NVT_EINVAL;
    }
    const uint8_t *body = r.p;
    if (h.compressed < 0 || h.uncompressed < 0 || (uint64_t)(end - body) < (uint64_t)h.compressed) {
      set_error("%s: page of %lld bytes runs past the chunk", w.who, (long long)h.compressed);
      return NVT_EINVAL;
    }
    p = body + h.compressed;   // the next page
    if (h.type == 1) continue;  // index page: nothing for us
    if (h.type == 2) {  // dictionary page: PLAIN values (encoding 0; 2 = PLAIN_DICTIONARY, the old name)
      if (have_dict || (h.dict_encoding != 0 && h.dict_encoding != 2) || !vs.takes_dictionary(h)) {
        set_error("%s: dictionary page (encoding %d, second %d)", w.who, h.dict_encoding, (int)have_dict);
        return NVT_EUNSUPPORTED;
      }
      const uint8_t *d = nullptr;
      if ((rc = page_bytes(w, body, (uint64_t)h.compressed, (uint64_t)h.uncompressed, w.codec != 0, 0, &d))) return rc;
      if ((rc = vs.dictionary(w.who, h, d))) return rc;
      have_dict = true;
      if (Values::kKeepsDictionary && w.codec != 0) scratch_at = ((uint64_t)h.uncompressed + 15) & ~15ull;
      continue;
    }
    if (h.type != 0 && h.type != 3) {
      set_error("%s: page type %d", w.who, h.type);
      return NVT_EUNSUPPORTED;
    }
    if ((rc = vs.accepts(w.who, h, have_dict))) return rc;
    const uint64_t prow = (uint64_t)h.num_values;
    if (h.num_values < 0 || prow > w.expect_rows - rows) {
      set_error("%s: more rows than the row group holds", w.who);
      return NVT_EINVAL;
    }
    // v2: repetition levels, then definition levels -- never compressed, no length prefix --, then
    // the values (compressed when the header says so)
    uint64_t lbytes = 0;
    if (h.type == 3) {
      if (h.rep_bytes != 0 && !Levels::kNested) {
        set_error("%s: repetition levels (nested column)", w.who);
        return NVT_EUNSUPPORTED;
      }
      // (each length is checked on its own before the sum: both are below 2^63 then)
      if (h.def_bytes < 0 || h.rep_bytes < 0 || (uint64_t)h.compressed < (uint64_t)h.def_bytes ||
          (uint64_t)h.uncompressed < (uint64_t)h.def_bytes || (uint64_t)h.compressed < (uint64_t)h.rep_bytes ||
          (uint64_t)h.uncompressed < (uint64_t)h.rep_bytes ||
          (uint64_t)h.compressed < (uint64_t)h.def_bytes + (uint64_t)h.rep_bytes ||
          (uint64_t)h.uncompressed < (uint64_t)h.def_bytes + (uint64_t)h.rep_bytes) {
        set_error("%s: definition levels run past the page", w.who);
        return NVT_EINVAL;
      }
      lbytes = (uint64_t)h.rep_bytes + (uint64_t)h.def_bytes;
    }
    const uint8_t *q = nullptr, *pend = nullptr;   // the values (behind the levels), uncompressed
    uint64_t pvalid = prow;
    if (w.codec == 1 && prow > 0 && vs.stays_compressed(h, lbytes, prow)) {
      // the body (v2: its values region) as it is; a v1 body still holds its levels in front
      lv.all_valid(rows, prow);
      rc = vs.compressed_page(w.who, h, body + lbytes, (uint64_t)h.compressed - lbytes, prow);
    } else {
      if (h.type == 0) {   // v1: u32 length | levels per stream, then the values, compressed together
        if ((rc = page_bytes(w, body, (uint64_t)h.compressed, (uint64_t)h.uncompressed, w.codec != 0, scratch_at, &q)))
          return rc;
        pend = q + h.uncompressed;
        if ((rc = lv.v1_encodings(w.who, h))) return rc;
      }
      const uint8_t *lp = body;
      for (int s = 0; s < 2; ++s) {
        if (!lv.has(s)) continue;
        uint64_t lb = s == 0 ? (uint64_t)h.rep_bytes : (uint64_t)h.def_bytes;
        if (h.type == 0) {
          uint32_t l32 = 0;
          if (pend - q >= 4) memcpy(&l32, q, 4);
          if (pend - q < 4 || (uint64_t)(pend - q - 4) < l32) {
            set_error("%s: page too short for its level streams", w.who);
            return NVT_EINVAL;
          }
          lp = q + 4;
          lb = l32;
          q = lp + lb;
        } else if (s == 1) {
          lp = body + h.rep_bytes;
        }
        if ((rc = lv.stream(w.who, s, lp, lb, rows, prow, &pvalid))) return rc;
      }
      if (h.type == 3) {
        if ((rc = page_bytes(w, body + lbytes, (uint64_t)h.compressed - lbytes, (uint64_t)h.uncompressed - lbytes,
                             w.codec != 0 && h.v2_compressed, scratch_at, &q)))
          return rc;
        pend = q + ((uint64_t)h.uncompressed - lbytes);
      }
      rc = vs.page(w.who, h, q, pend, pvalid);
    }
    if (rc) return rc;
    rows += prow;
  }
  if (rows != w.expect_rows) {
    set_error("%s: %llu rows in the pages, %llu expected", w.who, (unsigned long long)rows,
              (unsigned long long)w.expect_rows);
    return NVT_EINVAL;
  }
  return lv.close(w.who);
}

}  // namespace nvt
