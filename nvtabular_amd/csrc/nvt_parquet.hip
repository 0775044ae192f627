// Parquet in: the input half of Dataset -> HBM.  Reference contract: merlin.io.Dataset(engine=
// "parquet") feeding Workflow.fit / transform (tests/unit/workflow/test_cpu_workflow.py:67-81,
// bench/examples/dask-nvtabular-criteo-benchmark.py:216-237); the reference's backend (cuDF /
// pyarrow) decodes pages on its side of that call.
//
// Host (a pool thread per column, GIL released): pread a column chunk, then ONE walk over its pages
// (walk_pages, nvt_pq_page.hpp): thrift-compact page headers, bounds, codec UNCOMPRESSED / SNAPPY,
// data pages v1 / v2 split into levels and values, row accounting.  The walk hands the levels to a
// level sink and the dictionary page and the values to a value sink; every entry point is a pair of
// sinks.  Anything else in a chunk (other codecs / encodings, other nesting) is NVT_EUNSUPPORTED and
// the caller reads that file with pyarrow.  Device: values and bitmap arrive by hipMemcpyAsync; a
// column WITH nulls is expanded to one slot per row there (nvt_expand_valid below: rank of a row =
// popcount prefix of the bitmap), so the PCIe link carries the packed values only.
//
//   entry point                  level sink   value sink     device counterpart
//   nvt_pq_decode_chunk[_codec]  FlatLevels   PlainValues    nvt_expand_valid (here)
//   nvt_pq_decode_list_chunk     ListLevels   PlainValues    nvt_pqlist_unpack (nvt_parquet_list.hip)
//   nvt_pq_decode_chunk_delta    FlatLevels   DeltaValues    nvt_pq_delta_decode (nvt_parquet_delta.hip)
//   nvt_pq_decode_chunk_dict     FlatLevels   DictValues     nvt_pq_dict_fill_many (nvt_parquet_dict_in.hip)
//   nvt_pq_decode_chunk_inflate  FlatLevels   InflateValues  nvt_snappy_inflate_pages (nvt_snappy_inflate.hip)
//   nvt_pq_decode_bool_chunk     FlatLevels   BoolValues     nvt_expand_narrow (nvt_parquet_narrow.hip)
//   nvt_pq_decode_str_chunk      FlatLevels   StrValues (nvt_parquet_str_in.hip)
//                                                            nvt_pq_expand_runs (nvt_parquet_str.hip)
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_internal.hpp"
#include "nvt_pq_page.hpp"
#include "nvt_prof.hpp"
#include "nvt_scan.hpp"

namespace nvt {
namespace {

// ---- list columns: the level sink ("List columns in the parquet reader") --------------
// Repetition and definition levels of the pages -> the partition's two staging streams, from slot
// `slot0` on (the walk's rows are SLOTS); counts the row starts and the leaf slots on the way.
struct ListLevels {
  static constexpr bool kNested = true;
  uint8_t *rep, *def;          // the partition's staging streams
  uint64_t slot0;              // the chunk's first slot
  unsigned width;              // bits per definition level (1 or 2)
  unsigned leaf_level, max_def;
  uint64_t expect_rows;
  uint64_t starts = 0, leaves = 0;
  const char *bad_args() const { return rep && def ? nullptr : "null pointer"; }
  bool has(int) const { return true; }
  int v1_encodings(const char *who, const PageHead &h) const {
    if (h.rep_encoding == 3 && h.def_encoding == 3) return NVT_OK;
    set_error("%s: level encodings %d / %d (the RLE hybrid is decoded here)", who, h.rep_encoding, h.def_encoding);
    return NVT_EUNSUPPORTED;
  }
  int stream(const char *who, int s, const uint8_t *lv, uint64_t nbytes, uint64_t slot, uint64_t n, uint64_t *pvalid) {
    uint64_t hist[4] = {0, 0, 0, 0};
    const int bad = s == 0 ? decode_levels_wide(lv, nbytes, n, 1, 1, rep, slot0 + slot, hist)
                           : decode_levels_wide(lv, nbytes, n, width, max_def, def, slot0 + slot, hist);
    if (bad) {
      set_error(bad == 1 ? "%s: level runs leave their stream" : "%s: a level above the column's maximum", who);
      return NVT_EINVAL;
    }
    if (s == 0) {
      starts += hist[0];
      return NVT_OK;
    }
    *pvalid = hist[max_def];
    for (unsigned v = leaf_level; v <= max_def; ++v) leaves += hist[v];
    if (slot == 0 && n > 0 && ((rep[slot0 >> 3] >> (slot0 & 7)) & 1)) {
      set_error("%s: the chunk's first slot continues a row", who);
      return NVT_EINVAL;
    }
    return NVT_OK;
  }
  void all_valid(uint64_t, uint64_t) {}
  int close(const char *who) {
    if (starts == expect_rows) return NVT_OK;
    set_error("%s: %llu row starts in the pages, %llu expected", who, (unsigned long long)starts,
              (unsigned long long)expect_rows);
    return NVT_EINVAL;
  }
};

// ---- DELTA_BINARY_PACKED pages: staged, not decoded ("DELTA_BINARY_PACKED in the parquet
// reader") ---------------------------------------------------------------------------------------
// the fill state of a nvt_pq_delta_stage during one chunk: committed to the stage on NVT_OK only, so
// a chunk that asked for larger buffers is decoded again from its first byte
struct DeltaFill {
  nvt_pq_delta_stage *st;
  uint64_t nbytes, npages, nmbs;
  uint64_t *need;
  bool ints;   // the column's physical type is INT32 / INT64
  int grow(int which, uint64_t want) {
    need[0] = need[1] = need[2] = 0;
    need[which] = want;
    return NVT_PQ_DELTA_GROW;
  }
};

// One values region [q, q + nbytes) of `count` values at `type_size` bytes, the page's first value at
// `pos` of the column's packed values: one page record, one record per needed miniblock, and the
// region's bytes up to the end of the last needed miniblock.  Every header of the region is read
// here, once per block; what the device later reads is exactly what this walk has seen inside the
// region.
int delta_stage_page(DeltaFill &f, const uint8_t *q, uint64_t nbytes, int type_size, uint64_t count, uint64_t pos) {
  nvt_pq_delta_stage *st = f.st;
  TReader r{q, q + nbytes};
  const uint64_t block_size = r.varint(), mpb = r.varint(), total = r.varint();
  const int64_t first = r.zigzag();
  if (!r.ok) {
    set_error("nvt_pq_decode_chunk_delta: the header of a delta page runs past the page");
    return NVT_EINVAL;
  }
  if (block_size == 0 || block_size % 128 || mpb == 0 || block_size % mpb || (block_size / mpb) % 32 ||
      block_size > (1ull << 31)) {
    set_error("nvt_pq_decode_chunk_delta: blocks of %llu values in %llu miniblocks (a multiple of 128, miniblocks "
              "of a multiple of 32)", (unsigned long long)block_size, (unsigned long long)mpb);
    return NVT_EINVAL;
  }
  const uint64_t vpm = block_size / mpb;
  if (vpm > NVT_PQ_DELTA_TILE) {
    set_error("nvt_pq_decode_chunk_delta: miniblocks of %llu values (up to %u are decoded here)",
              (unsigned long long)vpm, NVT_PQ_DELTA_TILE);
    return NVT_EUNSUPPORTED;
  }
  if (total != count) {
    set_error("nvt_pq_decode_chunk_delta: a delta page of %llu values, its levels say %llu",
              (unsigned long long)total, (unsigned long long)count);
    return NVT_EINVAL;
  }
  if (count == 0) return NVT_OK;
  if (count >= (1ull << 32)) {
    set_error("nvt_pq_decode_chunk_delta: a page of %llu values", (unsigned long long)count);
    return NVT_EINVAL;
  }
  const uint64_t nmb = (count - 1 + vpm - 1) / vpm;
  if (f.npages + 1 > st->pages_cap) return f.grow(1, f.npages + 1);
  if (f.nmbs + nmb > st->mbs_cap) return f.grow(2, f.nmbs + nmb);
  uint64_t *rec = st->mbs + 2 * f.nmbs;
  for (uint64_t done = 0; done < nmb;) {
    const int64_t min_delta = r.zigzag();
    const uint8_t *widths = r.p;
    r.skip_bytes(mpb);
    if (!r.ok) {
      set_error("nvt_pq_decode_chunk_delta: a block header runs past its page");
      return NVT_EINVAL;
    }
    for (uint64_t m = 0; m < mpb && done < nmb; ++m, ++done, rec += 2) {
      const uint64_t w = widths[m];
      if (w > 8ull * (uint64_t)type_size) {
        set_error("nvt_pq_decode_chunk_delta: a miniblock of bit width %llu in a column of %d bits",
                  (unsigned long long)w, 8 * type_size);
        return NVT_EINVAL;
      }
      const uint64_t nb = vpm * w / 8;   // (the last needed miniblock is padded to full length)
      if ((uint64_t)(r.end - r.p) < nb) {
        set_error("nvt_pq_decode_chunk_delta: a miniblock runs past its page");
        return NVT_EINVAL;
      }
      rec[0] = (f.nbytes + (uint64_t)(r.p - q)) | (w << 56);
      rec[1] = (uint64_t)min_delta;
      r.p += nb;
    }
  }
  const uint64_t used = (uint64_t)(r.p - q);
  if (f.nbytes + used + 16 > st->bytes_cap) return f.grow(0, f.nbytes + used + 16);   // (far below 2^56)
  memcpy(st->bytes + f.nbytes, q, used);
  memset(st->bytes + f.nbytes + used, 0, 16);
  uint64_t *pg = st->pages + NVT_PQ_DELTA_RECORD_WORDS * f.npages;
  pg[0] = (uint64_t)first;
  pg[1] = pos;
  pg[2] = count | (vpm << 32);
  pg[3] = f.nmbs;
  pg[4] = f.nbytes;
  f.nbytes += used;
  f.npages += 1;
  f.nmbs += nmb;
  return NVT_OK;
}

// ---- snappy bodies of PLAIN pages: staged, not inflated ("Snappy pages in the parquet
// reader") ---------------------------------------------------------------------------------------
// the fill state of a nvt_pq_inflate_stage during one chunk: committed to the stage on NVT_OK only, so
// a chunk that asked for larger buffers is decoded again from its first byte
struct InflateFill {
  nvt_pq_inflate_stage *st;
  uint64_t nbytes, npages;
  uint64_t *need;
  int64_t chunk_nulls;   // the footer's null_count of the chunk, -1: it has none
  // one compressed body on a 16-byte boundary and its record
  int page(const uint8_t *body, uint64_t n, uint64_t dst_at, uint64_t dst_bytes, uint32_t flags) {
    const uint64_t at = (nbytes + 15) & ~15ull;
    need[0] = need[1] = 0;
    if (at + n > st->bytes_cap) {
      need[0] = at + n;
      return NVT_PQ_INFLATE_GROW;
    }
    if (npages + 1 > st->pages_cap) {
      need[1] = npages + 1;
      return NVT_PQ_INFLATE_GROW;
    }
    memset(st->bytes + nbytes, 0, at - nbytes);
    memcpy(st->bytes + at, body, n);
    st->pages[npages++] = nvt_inflate_page{at, n, dst_at, dst_bytes, flags, 0};
    nbytes = at + n;
    return NVT_OK;
  }
};

}  // namespace

// ---- snappy, raw block format (what parquet's SNAPPY codec holds per page; declared in
// nvt_pq_page.hpp for the walk) -------------------------------------------------------------------
// -> uncompressed bytes written, or -1 on malformed input / a block that does not fit `cap`
int64_t snappy_uncompress(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap) {
  TReader r{src, src + n};
  const uint64_t want = r.varint();
  if (!r.ok || want > cap) return -1;
  const uint8_t *p = r.p, *end = src + n;
  uint64_t o = 0;
  while (p < end) {
    const uint8_t tag = *p++;
    uint64_t len, off;
    switch (tag & 3) {
      case 0: {   // literal
        len = (uint64_t)(tag >> 2) + 1;
        if (len > 60) {
          const unsigned nb = (unsigned)(len - 60);   // 1 .. 4 length bytes, little endian
          if ((uint64_t)(end - p) < nb) return -1;
          len = 0;
          for (unsigned i = 0; i < nb; ++i) len |= (uint64_t)p[i] << (8 * i);
          len += 1;
          p += nb;
        }
        if ((uint64_t)(end - p) < len || want - o < len) return -1;
        memcpy(dst + o, p, len);
        p += len;
        o += len;
        continue;
      }
      case 1:
        if (p >= end) return -1;
        len = (uint64_t)((tag >> 2) & 7) + 4;
        off = ((uint64_t)(tag >> 5) << 8) | *p++;
        break;
      case 2:
        if (end - p < 2) return -1;
        len = (uint64_t)(tag >> 2) + 1;
        off = (uint64_t)p[0] | ((uint64_t)p[1] << 8);
        p += 2;
        break;
      default:
        if (end - p < 4) return -1;
        len = (uint64_t)(tag >> 2) + 1;
        off = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24);
        p += 4;
    }
    if (off == 0 || off > o || want - o < len) return -1;
    if (off >= len) {
      memcpy(dst + o, dst + o - off, len);
    } else {   // overlapping copy: a run
      for (uint64_t i = 0; i < len; ++i) dst[o + i] = dst[o - off + i];
    }
    o += len;
  }
  return o == want ? (int64_t)o : -1;
}

namespace {

// `count` dictionary indices (RLE / bit-packed hybrid behind a one-byte bit width) resolved through
// `dict` (ndict values of T) into out[0 .. count)
template <typename T>
bool decode_dict_indices(const uint8_t *p, const uint8_t *end, uint64_t count, const T *dict, uint64_t ndict,
                         T *out) {
  if (count == 0) return true;
  if (p >= end) return false;
  const unsigned bw = *p++;
  if (bw > 32) return false;
  const uint64_t mask = bw == 32 ? 0xFFFFFFFFull : ((1ull << bw) - 1ull);
  TReader r{p, end};
  uint64_t done = 0;
  while (done < count) {
    const uint64_t head = r.varint();
    if (!r.ok) return false;
    if (head & 1) {   // bit-packed: (head >> 1) groups of 8 values, `bw` bits each, LSB first
      const uint64_t groups = head >> 1;
      if (groups == 0 || groups > (1ull << 40)) return false;
      const uint64_t nb = groups * bw;
      if ((uint64_t)(r.end - r.p) < nb) {
        // (writers may truncate the padding of the last group: take what the values need)
        const uint64_t need_vals = count - done < groups * 8 ? count - done : groups * 8;
        if ((uint64_t)(r.end - r.p) * 8 < need_vals * bw) return false;
      }
      uint64_t take = groups * 8;
      if (take > count - done) take = count - done;
      const uint8_t *q = r.p;
      const uint64_t avail = (uint64_t)(r.end - r.p);
      uint64_t bitpos = 0;
      for (uint64_t i = 0; i < take; ++i, bitpos += bw) {
        const uint64_t byte = bitpos >> 3;
        uint64_t w = 0;   // up to 5 bytes hold a value of <= 32 bits at any bit offset
        if (avail - byte >= 8) memcpy(&w, q + byte, 8);   // (a fixed size: one load)
        else memcpy(&w, q + byte, avail - byte);
        const uint64_t idx = (w >> (bitpos & 7)) & mask;
        if (idx >= ndict) return false;
        out[done + i] = dict[idx];
      }
      r.skip_bytes(nb < avail ? nb : avail);
      done += take;
    } else {   // RLE: (head >> 1) times the value in the next ceil(bw / 8) bytes
      uint64_t n = head >> 1;
      const unsigned vb = (bw + 7) / 8;
      if (n == 0 || (uint64_t)(r.end - r.p) < vb) return false;
      uint64_t idx = 0;
      memcpy(&idx, r.p, vb);
      r.p += vb;
      idx &= mask;
      if (idx >= ndict) return false;
      if (n > count - done) n = count - done;
      const T v = dict[idx];
      for (uint64_t i = 0; i < n; ++i) out[done + i] = v;
      done += n;
    }
  }
  return true;
}

// ---- dictionary pages of number columns: staged, not resolved ("Dictionary pages of
// number columns in the parquet reader") -----------------------------------------------------------
// the fill state of a nvt_pq_dict_stage during one chunk: committed to the stage on NVT_OK only, so a
// chunk that asked for larger buffers is decoded again from its first byte
struct DictFill {
  nvt_pq_dict_stage *st;
  uint64_t ndict_bytes, nruns, npacked;
  uint64_t *need;
  uint64_t base = 0;   // entry position of the chunk's first dictionary entry
  int grow(int which, uint64_t want) {
    need[0] = need[1] = need[2] = 0;
    need[which] = want;
    return NVT_PQ_DICT_GROW;
  }
  // the chunk's dictionary (ndict PLAIN values of type_size bytes) behind a head, on a 16-byte boundary
  int dictionary(const uint8_t *d, uint64_t ndict, int type_size) {
    const uint64_t at = (ndict_bytes + 15) & ~15ull, nb = ndict * (uint64_t)type_size;
    if (at + NVT_PQ_DICT_HEAD_BYTES + nb > st->dict_cap) return grow(0, at + NVT_PQ_DICT_HEAD_BYTES + nb);
    if ((at + NVT_PQ_DICT_HEAD_BYTES + nb) / (uint64_t)type_size >= (1ull << 31)) {
      set_error("nvt_pq_decode_chunk_dict: 2^31 dictionary entries or more in one partition");
      return NVT_EUNSUPPORTED;
    }
    memset(st->dict + ndict_bytes, 0, at - ndict_bytes);
    const uint64_t head[2] = {ndict, 0};
    memcpy(st->dict + at, head, sizeof head);
    memcpy(st->dict + at + NVT_PQ_DICT_HEAD_BYTES, d, nb);
    base = (at + NVT_PQ_DICT_HEAD_BYTES) / (uint64_t)type_size;
    ndict_bytes = at + NVT_PQ_DICT_HEAD_BYTES + nb;
    return NVT_OK;
  }
  // one record {start, kind | width << 8, a, b} of `count` values; a repeat run that continues the
  // last record's entry and a KEEP run behind a KEEP run add nothing: a run ends where the next starts
  int run(unsigned kind, unsigned width, uint32_t a, uint32_t b, uint64_t start, uint64_t count) {
    if (count == 0) return NVT_OK;
    if (start + count >= (1ull << 32) - NVT_PQ_DICT_TILE) {
      set_error("nvt_pq_decode_chunk_dict: 2^32 values or more in one partition");
      return NVT_EUNSUPPORTED;
    }
    uint32_t *rec = st->runs + 4 * nruns;
    if (nruns > 0 && kind != NVT_PQ_RUN_PACKED && rec[-3] == kind && (kind == NVT_PQ_RUN_KEEP || rec[-2] == a))
      return NVT_OK;
    if (nruns + 2 > st->runs_cap) return grow(1, nruns + 2);   // (this record and the closing one)
    rec[0] = (uint32_t)start;
    rec[1] = kind | (width << 8);
    rec[2] = a;
    rec[3] = b;
    ++nruns;
    return NVT_OK;
  }
};

// the dictionary indices of one page (`count` non-null values from packed value `start` on; one byte
// bit width, then the RLE / bit-packed hybrid) -> run records; the bytes of bit-packed runs go to the
// packed staging buffer, each run's on a 4-byte boundary.  Refuses what decode_dict_indices refuses,
// but for the indices inside bit-packed runs, which the device checks.
int dict_index_runs(DictFill &f, const uint8_t *p, const uint8_t *end, uint64_t count, uint64_t ndict,
                    uint64_t start) {
  if (count == 0) return NVT_OK;
  if (p >= end) return NVT_EINVAL;
  const unsigned bw = *p++;
  if (bw > 32) return NVT_EINVAL;
  const uint64_t mask = bw == 32 ? 0xFFFFFFFFull : ((1ull << bw) - 1ull);
  TReader r{p, end};
  uint64_t done = 0;
  while (done < count) {
    const uint64_t head = r.varint();
    if (!r.ok) return NVT_EINVAL;
    const uint64_t avail = (uint64_t)(r.end - r.p);
    if (head & 1) {   // bit-packed: (head >> 1) groups of 8 values, `bw` bits each, LSB first
      const uint64_t groups = head >> 1;
      if (groups == 0 || groups > (1ull << 40)) return NVT_EINVAL;
      uint64_t take = groups * 8;
      if (take > count - done) take = count - done;   // (the last group is padded)
      const uint64_t nb = (take * bw + 7) / 8;        // the bytes the values need
      if (avail < nb) return NVT_EINVAL;
      int rc;
      if (bw == 0) {   // a one-entry dictionary: every index is 0
        if (ndict == 0) return NVT_EINVAL;
        rc = f.run(NVT_PQ_RUN_REPEAT, 0, (uint32_t)f.base, 0, start + done, take);
      } else {
        const uint64_t at = (f.npacked + 3) & ~3ull;
        if (at + nb + 8 > f.st->packed_cap) return f.grow(2, at + nb + 8);
        if (at + nb + 8 >= (1ull << 34)) {
          set_error("nvt_pq_decode_chunk_dict: 16 GiB or more of packed indices in one partition");
          return NVT_EUNSUPPORTED;
        }
        memset(f.st->packed + f.npacked, 0, at - f.npacked);
        memcpy(f.st->packed + at, r.p, nb);
        memset(f.st->packed + at + nb, 0, 8);
        f.npacked = at + nb;
        rc = f.run(NVT_PQ_RUN_PACKED, bw, (uint32_t)f.base, (uint32_t)(at / 4), start + done, take);
      }
      if (rc) return rc;
      r.skip_bytes(groups * bw < avail ? groups * bw : avail);   // (a writer may cut the padding)
      done += take;
    } else {   // RLE: (head >> 1) times the value in the next ceil(bw / 8) bytes
      uint64_t n = head >> 1;
      const unsigned vb = (bw + 7) / 8;
      if (n == 0 || avail < vb) return NVT_EINVAL;
      uint64_t idx = 0;
      memcpy(&idx, r.p, vb);
      r.p += vb;
      idx &= mask;
      if (idx >= ndict) return NVT_EINVAL;
      if (n > count - done) n = count - done;
      const int rc = f.run(NVT_PQ_RUN_REPEAT, 0, (uint32_t)(f.base + idx), 0, start + done, n);
      if (rc) return rc;
      done += n;
    }
  }
  return NVT_OK;
}

// ---- the value sinks of number columns -------------------------------------------------------------
// The default: PLAIN values are moved behind each other into `out` -- PLAIN stores only the non-null
// ones -- and dictionary indices resolved through the chunk's dictionary (in the chunk or at the
// bottom of the scratch), so `out` holds packed PLAIN values.
struct PlainValues : ValueSink {
  static constexpr bool kKeepsDictionary = true;
  int type_size;
  uint8_t *out;
  uint64_t cap_bytes;
  bool exact;   // list chunks: the levels say how many PLAIN values a page holds, exactly
  uint64_t vals = 0;
  const uint8_t *dict = nullptr;   // PLAIN values of the dictionary page
  uint64_t ndict = 0;
  PlainValues(int type_size_, uint8_t *out_, uint64_t cap_bytes_, bool exact_ = false)
      : type_size(type_size_), out(out_), cap_bytes(cap_bytes_), exact(exact_) {}
  bool takes_dictionary(const PageHead &h) const { return h.dict_values >= 0; }
  int dictionary(const char *who, const PageHead &h, const uint8_t *d) {
    // compared by division: a count of 2^61 must not wrap
    if ((uint64_t)h.dict_values > (uint64_t)h.uncompressed / (uint64_t)type_size) {
      set_error("%s: dictionary page holds fewer values than it says", who);
      return NVT_EINVAL;
    }
    dict = d;
    ndict = (uint64_t)h.dict_values;
    return NVT_OK;
  }
  int accepts(const char *who, const PageHead &h, bool have_dict) const { return plain_or_dictionary(who, h, have_dict); }
  int room(const char *who, uint64_t count) const {
    if ((vals + count) * (uint64_t)type_size <= cap_bytes) return NVT_OK;
    set_error("%s: values buffer too small", who);
    return NVT_EINVAL;
  }
  int page(const char *who, const PageHead &h, const uint8_t *q, const uint8_t *pend, uint64_t pvalid) {
    if (const int rc = room(who, pvalid)) return rc;
    if (by_dictionary(h)) {
      const bool ok = type_size == 4
          ? decode_dict_indices<uint32_t>(q, pend, pvalid, reinterpret_cast<const uint32_t *>(dict), ndict,
                                          reinterpret_cast<uint32_t *>(out) + vals)
          : decode_dict_indices<uint64_t>(q, pend, pvalid, reinterpret_cast<const uint64_t *>(dict), ndict,
                                          reinterpret_cast<uint64_t *>(out) + vals);
      if (!ok) {
        set_error("%s: malformed dictionary indices", who);
        return NVT_EINVAL;
      }
    } else {
      const uint64_t vbytes = pvalid * (uint64_t)type_size;
      if ((uint64_t)(pend - q) < vbytes) {
        set_error("%s: page holds fewer values than its levels say", who);
        return NVT_EINVAL;
      }
      if (exact && (uint64_t)(pend - q) != vbytes) {
        set_error("%s: page holds more values than its levels say", who);
        return NVT_EINVAL;
      }
      memcpy(out + vals * (uint64_t)type_size, q, vbytes);
    }
    vals += pvalid;
    return NVT_OK;
  }
};

// The three sinks that leave HOLES in `out` for the device to fill: what they stage goes to their
// fill, every other page is decoded in place as above.  `values_offset`: out[0] is this value of the
// column's packed values.
struct DeltaValues : PlainValues {   // DELTA_BINARY_PACKED pages (nvt_pq_delta_decode)
  DeltaFill f;
  uint64_t values_offset;
  DeltaValues(const PlainValues &base, const DeltaFill &f_, uint64_t values_offset_)
      : PlainValues(base), f(f_), values_offset(values_offset_) {}
  int accepts(const char *who, const PageHead &h, bool have_dict) const {
    if (h.encoding != 5) return PlainValues::accepts(who, h, have_dict);
    if (f.ints) return NVT_OK;
    set_error("%s: DELTA_BINARY_PACKED values in a column that is not INT32 / INT64", who);
    return NVT_EINVAL;
  }
  int page(const char *who, const PageHead &h, const uint8_t *q, const uint8_t *pend, uint64_t pvalid) {
    if (h.encoding != 5) return PlainValues::page(who, h, q, pend, pvalid);
    int rc = room(who, pvalid);
    if (!rc) rc = delta_stage_page(f, q, (uint64_t)(pend - q), type_size, pvalid, values_offset + vals);
    if (!rc) vals += pvalid;
    return rc;
  }
};

struct DictValues : PlainValues {   // dictionary-encoded pages (nvt_pq_dict_fill_many)
  DictFill f;
  uint64_t values_offset;
  DictValues(const PlainValues &base, const DictFill &f_, uint64_t values_offset_)
      : PlainValues(base), f(f_), values_offset(values_offset_) {}
  int dictionary(const char *who, const PageHead &h, const uint8_t *d) {
    const int rc = PlainValues::dictionary(who, h, d);
    return rc ? rc : f.dictionary(d, ndict, type_size);
  }
  int page(const char *who, const PageHead &h, const uint8_t *q, const uint8_t *pend, uint64_t pvalid) {
    const uint64_t start = values_offset + vals;
    if (!by_dictionary(h)) {   // in place: the device leaves these positions alone
      const int rc = PlainValues::page(who, h, q, pend, pvalid);
      return rc ? rc : f.run(NVT_PQ_RUN_KEEP, 0, 0, 0, start, pvalid);
    }
    int rc = room(who, pvalid);
    if (!rc) {
      rc = dict_index_runs(f, q, pend, pvalid, ndict, start);
      if (rc == NVT_EINVAL) set_error("%s: malformed dictionary indices", who);
    }
    if (!rc) vals += pvalid;
    return rc;
  }
};

struct InflateValues : PlainValues {   // snappy bodies of PLAIN pages without nulls (nvt_snappy_inflate_pages)
  InflateFill f;
  uint64_t values_offset;
  int max_def;
  InflateValues(const PlainValues &base, const InflateFill &f_, uint64_t values_offset_, int max_def_)
      : PlainValues(base), f(f_), values_offset(values_offset_), max_def(max_def_) {}
  // a non-empty snappy body of PLAIN values that is known to hold no nulls (the walk asks for SNAPPY
  // chunks and pages with rows only)
  bool stays_compressed(const PageHead &h, uint64_t lbytes, uint64_t prow) const {
    if (h.encoding != 0) return false;
    if (h.type == 0)   // (levels in another encoding than the RLE hybrid have no u32 L in front: left to the host)
      return h.compressed > 0 &&
             (max_def == 0 ||
              (h.def_encoding == 3 && (h.stat_nulls == 0 || (h.stat_nulls < 0 && f.chunk_nulls == 0))));
    return h.v2_compressed && (max_def == 0 || h.num_nulls == 0) && (uint64_t)h.compressed > lbytes &&
           (uint64_t)h.uncompressed - lbytes == prow * (uint64_t)type_size;
  }
  // v1: the levels (u32 L | L bytes) are inside the body; the device drops them
  int compressed_page(const char *who, const PageHead &h, const uint8_t *body, uint64_t n, uint64_t prow) {
    int rc = room(who, prow);
    if (!rc)
      rc = f.page(body, n, (values_offset + vals) * (uint64_t)type_size, prow * (uint64_t)type_size,
                  (h.type == 0 && max_def == 1) ? NVT_INFLATE_V1_LEVELS : 0u);
    if (!rc) vals += prow;
    return rc;
  }
};

// One chunk of a number column through the walk: the argument checks and outputs that its entry
// points share.  *rows_out counts what w.expect_rows counts.
template <typename Levels, typename Values>
int decode_numbers(const PageWalk &w, Levels &lv, Values &vs, uint64_t *rows_out, uint64_t *values_count) {
  const char *bad = !(w.chunk && vs.out && rows_out && values_count) ? "null pointer"
                    : (vs.type_size != 4 && vs.type_size != 8)      ? "values are 4 or 8 bytes"
                                                                     : lv.bad_args();
  if (bad) {
    set_error("%s: %s", w.who, bad);
    return NVT_EINVAL;
  }
  const int rc = walk_pages(w, lv, vs);
  if (rc) return rc;
  *rows_out = w.expect_rows;
  *values_count = vs.vals;
  return NVT_OK;
}

}  // namespace

// out[i] = valid(i) ? packed[rank(i)] : 0 with rank(i) = valid rows in front of row i.
// A wave takes 64 bitmap words (4096 rows): lane l owns word l for the rank prefix, then the
// wave walks the 64 words, lane r writing row 64 * w + r -- coalesced stores, and the loads of
// the packed values are consecutive too.
constexpr int kExpWaveRows = 64 * 64;
template <typename T>
__global__ __launch_bounds__(kBlock) void expand_valid_kernel(const T *__restrict__ packed,
                                                              const uint64_t *__restrict__ bitmap,
                                                              uint64_t n,
                                                              const unsigned *__restrict__ tile_base,
                                                              T *__restrict__ out) {
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const uint64_t nwords = (n + 63) / 64;
  const uint64_t w0 = wave * 64;
  if (w0 >= nwords) return;
  uint64_t word = (w0 + lane < nwords) ? bitmap[w0 + lane] : 0ull;
  const uint64_t row0 = (w0 + lane) * 64;
  if (row0 + 64 > n) word &= row0 >= n ? 0ull : ((1ull << (n - row0)) - 1ull);  // bits behind the column
  const unsigned pc = (unsigned)__popcll(word);
  unsigned inc = pc;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += o;
  }
  const uint64_t wbase = (uint64_t)tile_base[wave] + inc - pc;  // valid rows in front of word `lane`
  for (int w = 0; w < 64; ++w) {
    if (w0 + w >= nwords) break;  // (uniform)
    const uint64_t bits = __shfl(word, w, 64);
    const uint64_t base = __shfl(wbase, w, 64);
    const uint64_t row = (w0 + w) * 64 + lane;
    if (row < n) {
      const bool v = (bits >> lane) & 1ull;
      const uint64_t rank = base + (uint64_t)__popcll(bits & ((1ull << lane) - 1ull));
      out[row] = v ? packed[rank] : (T)0;
    }
  }
}

__global__ __launch_bounds__(kBlock) void expand_count_kernel(const uint64_t *__restrict__ bitmap, uint64_t n,
                                                              unsigned *__restrict__ tile_cnt, uint64_t ntiles) {
  const unsigned lane = lane_id();
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (wave >= ntiles) return;
  const uint64_t nwords = (n + 63) / 64;
  const uint64_t wi = wave * 64 + lane;
  uint64_t word = wi < nwords ? bitmap[wi] : 0ull;
  const uint64_t row0 = wi * 64;
  if (row0 + 64 > n) word &= row0 >= n ? 0ull : ((1ull << (n - row0)) - 1ull);
  unsigned pc = (unsigned)__popcll(word);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) pc += __shfl_down(pc, off, 64);
  if (lane == 0) tile_cnt[wave] = pc;
}

}  // namespace nvt

using namespace nvt;

extern "C" {

int nvt_pq_decode_list_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size,
                             int leaf_level, int max_def_level, uint64_t expect_slots, uint64_t expect_rows,
                             uint8_t *rep_out, uint8_t *def_out, uint64_t slot_offset, uint64_t slot_cap,
                             uint8_t *values_out, uint64_t values_cap_bytes, uint8_t *scratch,
                             uint64_t scratch_bytes, uint64_t *counts) {
  NVT_CHECK_ARG(rep_out && def_out && counts, "null pointer");
  NVT_CHECK_ARG(leaf_level == 1 || leaf_level == 2, "leaf_level is 1 or 2 (required / optional outer group)");
  NVT_CHECK_ARG(max_def_level == leaf_level || max_def_level == leaf_level + 1,
                "max_def_level is leaf_level (+ 1 for optional leaves)");
  NVT_CHECK_ARG(slot_offset <= slot_cap && expect_slots <= slot_cap - slot_offset, "the slots do not fit the level streams");
  NVT_CHECK_ARG(slot_cap < (1ull << 60), "slot_cap too large");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_slots, scratch, scratch_bytes};
  ListLevels lv{rep_out, def_out, slot_offset, max_def_level == 1 ? 1u : 2u, (unsigned)leaf_level,
                (unsigned)max_def_level, expect_rows};
  PlainValues vs(type_size, values_out, values_cap_bytes, true);
  uint64_t slots = 0, vals = 0;
  const int rc = decode_numbers(w, lv, vs, &slots, &vals);
  if (rc) return rc;
  counts[0] = slots;
  counts[1] = lv.starts;
  counts[2] = lv.leaves;
  counts[3] = vals;
  return NVT_OK;
}

int nvt_pq_decode_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int type_size, int max_def_level,
                        uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                        uint8_t *values_out, uint64_t values_cap_bytes, uint64_t *rows_out,
                        uint64_t *values_out_count) {
  const PageWalk w{__func__, chunk, chunk_bytes, 0, expect_rows, nullptr, 0};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  PlainValues vs(type_size, values_out, values_cap_bytes);
  return decode_numbers(w, lv, vs, rows_out, values_out_count);
}

int nvt_pq_decode_chunk_codec(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size,
                              int max_def_level, uint64_t expect_rows, uint8_t *valid_out,
                              uint64_t valid_bit_offset, uint8_t *values_out, uint64_t values_cap_bytes,
                              uint8_t *scratch, uint64_t scratch_bytes, uint64_t *rows_out,
                              uint64_t *values_out_count) {
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  PlainValues vs(type_size, values_out, values_cap_bytes);
  return decode_numbers(w, lv, vs, rows_out, values_out_count);
}

int nvt_pq_delta_stage_page(const uint8_t *region, uint64_t region_bytes, int type_size, uint64_t count,
                            uint64_t pos, nvt_pq_delta_stage *stage, uint64_t *need) {
  NVT_CHECK_ARG(region && stage && need, "null pointer");
  NVT_CHECK_ARG(type_size == 4 || type_size == 8, "values are 4 or 8 bytes");
  NVT_CHECK_ARG(stage->bytes && stage->pages && stage->mbs, "null staging buffer");
  DeltaFill f{stage, stage->nbytes, stage->npages, stage->nmbs, need, true};
  const int rc = delta_stage_page(f, region, region_bytes, type_size, count, pos);
  if (rc) return rc;
  stage->nbytes = f.nbytes;
  stage->npages = f.npages;
  stage->nmbs = f.nmbs;
  return NVT_OK;
}

int nvt_pq_decode_chunk_delta(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int ptype, int max_def_level,
                              uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                              uint8_t *values_out, uint64_t values_cap_bytes, uint64_t values_offset,
                              nvt_pq_delta_stage *stage, uint8_t *scratch, uint64_t scratch_bytes,
                              uint64_t *rows_out, uint64_t *values_count, uint64_t *need) {
  NVT_CHECK_ARG(stage && need, "null pointer");
  NVT_CHECK_ARG(ptype == 1 || ptype == 2 || ptype == 4 || ptype == 5, "physical type INT32, INT64, FLOAT or DOUBLE");
  NVT_CHECK_ARG(stage->bytes && stage->pages && stage->mbs, "null staging buffer");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  DeltaValues vs(PlainValues((ptype == 1 || ptype == 4) ? 4 : 8, values_out, values_cap_bytes),
                 DeltaFill{stage, stage->nbytes, stage->npages, stage->nmbs, need, ptype == 1 || ptype == 2},
                 values_offset);
  const int rc = decode_numbers(w, lv, vs, rows_out, values_count);
  if (rc) return rc;
  stage->nbytes = vs.f.nbytes;
  stage->npages = vs.f.npages;
  stage->nmbs = vs.f.nmbs;
  return NVT_OK;
}

int nvt_pq_decode_chunk_dict(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size, int max_def_level,
                             uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                             uint8_t *values_out, uint64_t values_cap_bytes, uint64_t values_offset,
                             nvt_pq_dict_stage *stage, uint8_t *scratch, uint64_t scratch_bytes,
                             uint64_t *rows_out, uint64_t *values_count, uint64_t *need) {
  NVT_CHECK_ARG(stage && need, "null pointer");
  NVT_CHECK_ARG(stage->dict && stage->runs && stage->packed, "null staging buffer");
  NVT_CHECK_ARG(stage->runs_cap >= 1 && stage->nruns < stage->runs_cap && stage->packed_cap >= 8 &&
                    stage->npacked <= stage->packed_cap - 8 && stage->ndict_bytes <= stage->dict_cap,
                "the stage's fill state does not fit its capacities");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  DictValues vs(PlainValues(type_size, values_out, values_cap_bytes),
                DictFill{stage, stage->ndict_bytes, stage->nruns, stage->npacked, need}, values_offset);
  const int rc = decode_numbers(w, lv, vs, rows_out, values_count);
  if (rc) return rc;
  const DictFill &f = vs.f;
  uint32_t *closing = stage->runs + 4 * f.nruns;   // (run() kept room for it)
  closing[0] = (uint32_t)(values_offset + *values_count);
  closing[1] = NVT_PQ_RUN_END;
  closing[2] = closing[3] = 0;
  stage->ndict_bytes = f.ndict_bytes;
  stage->nruns = f.nruns;
  stage->npacked = f.npacked;
  return NVT_OK;
}

int nvt_pq_decode_chunk_inflate(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int type_size,
                                int max_def_level, uint64_t expect_rows, uint8_t *valid_out,
                                uint64_t valid_bit_offset, uint8_t *values_out, uint64_t values_cap_bytes,
                                uint64_t values_offset, int64_t chunk_nulls, nvt_pq_inflate_stage *stage,
                                uint8_t *scratch, uint64_t scratch_bytes, uint64_t *rows_out,
                                uint64_t *values_count, uint64_t *need) {
  NVT_CHECK_ARG(stage && need, "null pointer");
  NVT_CHECK_ARG(stage->bytes && stage->pages, "null staging buffer");
  NVT_CHECK_ARG(stage->nbytes <= stage->bytes_cap && stage->npages <= stage->pages_cap,
                "the stage's fill state does not fit its capacities");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  InflateValues vs(PlainValues(type_size, values_out, values_cap_bytes),
                   InflateFill{stage, stage->nbytes, stage->npages, need, chunk_nulls}, values_offset, max_def_level);
  const int rc = decode_numbers(w, lv, vs, rows_out, values_count);
  if (rc) return rc;
  stage->nbytes = vs.f.nbytes;
  stage->npages = vs.f.npages;
  return NVT_OK;
}

// ---- bool columns: one bit per non-null value in the file, one byte each in the staging buffer
// ("Narrow and bool columns in the parquet path") ----------------------------------------
namespace {

// bits [0, count) of src (LSB first) -> one byte each
inline void bits_to_bytes(const uint8_t *src, uint64_t count, uint8_t *out) {
  for (uint64_t i = 0; i < count; ++i) out[i] = (uint8_t)((src[i >> 3] >> (i & 7)) & 1);
}

// `count` values of an RLE page (the hybrid at bit width 1 in [p, end)) -> one byte each.  A run is
// taken only if the page still owes its values: a repeat run longer than that, or a bit-packed run
// with a whole group more, is an error, like a run whose bytes leave the page.
bool decode_bool_rle(const uint8_t *p, const uint8_t *end, uint64_t count, uint8_t *out) {
  TReader r{p, end};
  uint64_t done = 0;
  while (done < count) {
    const uint64_t head = r.varint();
    if (!r.ok) return false;
    const uint64_t avail = (uint64_t)(r.end - r.p);
    if (head & 1) {
      const uint64_t groups = head >> 1;
      if (groups == 0 || groups > (count - done + 7) / 8) return false;   // (compared in groups: no product)
      uint64_t take = groups * 8;
      if (take > count - done) take = count - done;
      if (avail < (take + 7) / 8) return false;   // (a writer may cut the last group's padding, not its values)
      bits_to_bytes(r.p, take, out + done);
      r.skip_bytes(groups < avail ? groups : avail);
      done += take;
    } else {
      const uint64_t n = head >> 1;
      if (n == 0 || n > count - done || avail < 1) return false;
      const uint8_t v = *r.p++;
      if (v > 1) return false;
      memset(out + done, v, n);
      done += n;
    }
  }
  return true;
}

// the value sink: PLAIN bits or RLE runs -> one byte per non-null value.  Parquet has no bool
// dictionaries: a dictionary page is refused.
struct BoolValues : ValueSink {
  uint8_t *out;
  uint64_t cap;
  uint64_t vals = 0;
  BoolValues(uint8_t *out_, uint64_t cap_) : out(out_), cap(cap_) {}
  int accepts(const char *who, const PageHead &h, bool) const {
    if (h.encoding == 0 || h.encoding == 3) return NVT_OK;   // PLAIN (bit-packed) / RLE
    set_error("%s: value encoding %d (PLAIN and RLE are decoded here)", who, h.encoding);
    return NVT_EUNSUPPORTED;
  }
  int page(const char *who, const PageHead &h, const uint8_t *q, const uint8_t *pend, uint64_t pvalid) {
    if (pvalid > cap - vals) {
      set_error("%s: values buffer too small", who);
      return NVT_EINVAL;
    }
    if (h.encoding == 0) {
      if ((uint64_t)(pend - q) < (pvalid + 7) / 8) {
        set_error("%s: page holds fewer values than its levels say", who);
        return NVT_EINVAL;
      }
      bits_to_bytes(q, pvalid, out + vals);
    } else if (pvalid) {
      // RLE: u32 length | runs of the hybrid at bit width 1
      uint32_t lb = 0;
      if (pend - q >= 4) memcpy(&lb, q, 4);
      if (pend - q < 4 || (uint64_t)(pend - q - 4) < lb || !decode_bool_rle(q + 4, q + 4 + lb, pvalid, out + vals)) {
        set_error("%s: malformed RLE values", who);
        return NVT_EINVAL;
      }
    }
    vals += pvalid;
    return NVT_OK;
  }
};

}  // namespace

int nvt_pq_decode_bool_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int max_def_level,
                             uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                             uint8_t *values_out, uint64_t values_cap, uint8_t *scratch, uint64_t scratch_bytes,
                             uint64_t *rows_out, uint64_t *values_count) {
  NVT_CHECK_ARG(chunk && values_out && rows_out && values_count, "null pointer");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  NVT_CHECK_ARG(lv.bad_args() == nullptr, lv.bad_args());
  BoolValues vs(values_out, values_cap);
  const int rc = walk_pages(w, lv, vs);
  if (rc) return rc;
  *rows_out = expect_rows;
  *values_count = vs.vals;
  return NVT_OK;
}


int nvt_expand_valid_ws_bytes(uint64_t n, uint64_t *bytes) {
  NVT_CHECK_ARG(bytes, "null out");
  const uint64_t ntiles = (n + kExpWaveRows - 1) / kExpWaveRows;
  *bytes = ((ntiles * 4 + 255) & ~255ull) + scan_chunks(ntiles) * 8 + 256;
  return NVT_OK;
}

int nvt_expand_valid(const void *packed, int type_size, const uint8_t *bitmap, uint64_t n, void *out,
                     void *ws, void *stream) {
  if (n == 0) return NVT_OK;
  NVT_CHECK_ARG(packed && bitmap && out && ws, "null pointer");
  NVT_CHECK_ARG(type_size == 4 || type_size == 8, "values are 4 or 8 bytes");
  NVT_CHECK_ARG((reinterpret_cast<uintptr_t>(bitmap) & 7) == 0, "bitmap must be 8-byte aligned");
  NVT_CHECK_ARG(n < (1ull << 32), "fewer than 2^32 rows");
  hipStream_t s = (hipStream_t)stream;
  NVT_PROF("parquet_expand", n * (uint64_t)type_size, s);
  const uint64_t ntiles = (n + kExpWaveRows - 1) / kExpWaveRows;
  unsigned *tile = reinterpret_cast<unsigned *>(ws);
  unsigned long long *chunk_tot =
      reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ws) + ((ntiles * 4 + 255) & ~255ull));
  const uint64_t *bm = reinterpret_cast<const uint64_t *>(bitmap);
  const unsigned grid = (unsigned)((ntiles + (kBlock / kWave) - 1) / (kBlock / kWave));
  expand_count_kernel<<<grid, kBlock, 0, s>>>(bm, n, tile, ntiles);
  NVT_CHECK_LAUNCH();
  int rc = exclusive_scan_u32(tile, ntiles, chunk_tot, s);
  if (rc) return rc;
  if (type_size == 4)
    expand_valid_kernel<uint32_t><<<grid, kBlock, 0, s>>>((const uint32_t *)packed, bm, n, tile, (uint32_t *)out);
  else
    expand_valid_kernel<uint64_t><<<grid, kBlock, 0, s>>>((const uint64_t *)packed, bm, n, tile, (uint64_t *)out);
  NVT_CHECK_LAUNCH();
  return NVT_OK;
}

}  // extern "C"
