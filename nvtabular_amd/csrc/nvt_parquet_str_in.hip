// Parquet in, string columns (flat BYTE_ARRAY annotated UTF8 / STRING; DESIGN.md, "String columns in
// the parquet reader"): nvt_pq_decode_str_chunk walks the pages like every other entry point
// (walk_pages, nvt_pq_page.hpp) but expands nothing: dictionary and PLAIN values become entries of an
// Arrow string table, the index streams a run table plus the bytes of their bit-packed runs; the
// device expands the runs to entry ids (nvt_pq_expand_runs, nvt_parquet_str.hip) and hashes every
// entry once.  Host code only.
#include <string.h>

#include "../../include/nvt_hip.h"
#include "nvt_common.hpp"
#include "nvt_pq_page.hpp"

namespace nvt {
namespace {

// the fill state of a nvt_pq_str_stage during one chunk: committed to the stage on NVT_OK only, so a
// chunk that asked for larger buffers is decoded again from its first byte
struct StrFill {
  nvt_pq_str_stage *st;
  uint64_t entries, nchars, nruns, npacked, nvalues;
  uint64_t *need;
  // -> NVT_OK, or NVT_PQ_STR_GROW with need[which] = the least capacity that would have sufficed here
  int room(int which, uint64_t want, uint64_t cap) {
    if (want <= cap) return NVT_OK;
    need[which] = want;
    set_error("nvt_pq_decode_str_chunk: staging buffer %d holds %llu, %llu needed", which, (unsigned long long)cap,
              (unsigned long long)want);
    return NVT_PQ_STR_GROW;
  }
  // one record [start = nvalues, kind | width << 8, a, b]; a repeat run that continues the last
  // record's entry, or a sequence that continues its entries, adds nothing: a run ends where the next
  // record starts
  int run(unsigned kind, unsigned width, uint32_t a, uint32_t b, uint64_t count) {
    if (count == 0) return NVT_OK;
    uint32_t *rec = st->runs + 4 * nruns;
    bool merged = false;
    if (nruns > 0) {
      const uint32_t *last = rec - 4;
      if (kind == NVT_PQ_RUN_REPEAT && last[1] == NVT_PQ_RUN_REPEAT && last[2] == a) merged = true;
      if (kind == NVT_PQ_RUN_SEQUENCE && last[1] == NVT_PQ_RUN_SEQUENCE &&
          (uint64_t)last[2] + (nvalues - last[0]) == (uint64_t)a)
        merged = true;
    }
    if (!merged) {
      const int rc = room(2, nruns + 2, st->runs_cap);   // (this record and the closing one)
      if (rc) return rc;
      rec[0] = (uint32_t)nvalues;
      rec[1] = kind | (width << 8);
      rec[2] = a;
      rec[3] = b;
      ++nruns;
    }
    nvalues += count;
    return NVT_OK;
  }
};

// `count` PLAIN BYTE_ARRAY values (u32 length | bytes, each) in [q, pend) -> appended entries
int str_append_plain(StrFill &f, const uint8_t *q, const uint8_t *pend, uint64_t count) {
  int rc = f.room(0, f.entries + count, f.st->entries_cap);
  if (rc) return rc;
  for (uint64_t i = 0; i < count; ++i) {
    if ((uint64_t)(pend - q) < 4) {
      set_error("nvt_pq_decode_str_chunk: a length prefix past its page");
      return NVT_EINVAL;
    }
    uint32_t len;
    memcpy(&len, q, 4);
    q += 4;
    if ((uint64_t)(pend - q) < len) {
      set_error("nvt_pq_decode_str_chunk: a value of %u bytes runs past its page", len);
      return NVT_EINVAL;
    }
    if ((rc = f.room(1, ((f.nchars + len + 3) & ~3ull), f.st->chars_cap))) return rc;
    memcpy(f.st->chars + f.nchars, q, len);
    q += len;
    f.nchars += len;
    f.st->offsets[++f.entries] = (int64_t)f.nchars;
  }
  return NVT_OK;
}

// the dictionary indices of one page (`count` non-null values; one byte bit width, then the RLE /
// bit-packed hybrid) -> run records; the bytes of bit-packed runs go to the packed staging buffer,
// each run's on a 4-byte boundary
int str_index_runs(StrFill &f, const uint8_t *p, const uint8_t *end, uint64_t count, uint64_t base,
                   uint64_t ndict) {
  if (count == 0) return NVT_OK;
  if (p >= end) {
    set_error("nvt_pq_decode_str_chunk: an index page without its bit width");
    return NVT_EINVAL;
  }
  const unsigned bw = *p++;
  if (bw > 32) {
    set_error("nvt_pq_decode_str_chunk: dictionary indices of bit width %u", bw);
    return NVT_EINVAL;
  }
  const uint32_t kBadId = 0xFFFFFFFFu;   // (entries stay below 2^31: the device counts this id as bad)
  if (bw == 0)   // a one-entry dictionary: every value is its entry, whatever runs the page spells out
    return f.run(NVT_PQ_RUN_REPEAT, 0, ndict ? (uint32_t)base : kBadId, 0, count);
  const uint64_t mask = bw == 32 ? 0xFFFFFFFFull : ((1ull << bw) - 1ull);
  TReader r{p, end};
  uint64_t done = 0;
  while (done < count) {
    const uint64_t head = r.varint();
    if (!r.ok) {
      set_error("nvt_pq_decode_str_chunk: the index runs end before the page's values");
      return NVT_EINVAL;
    }
    const uint64_t avail = (uint64_t)(r.end - r.p);
    if (head & 1) {   // bit-packed: (head >> 1) groups of 8 values, `bw` bits each, LSB first
      const uint64_t groups = head >> 1;
      if (groups > (1ull << 40)) {
        set_error("nvt_pq_decode_str_chunk: a bit-packed run of %llu groups", (unsigned long long)groups);
        return NVT_EINVAL;
      }
      uint64_t take = groups * 8;
      if (take > count - done) take = count - done;   // (the last group is padded)
      const uint64_t nb = (take * bw + 7) / 8;        // the bytes the values need
      if (avail < nb) {
        set_error("nvt_pq_decode_str_chunk: a bit-packed run past its page");
        return NVT_EINVAL;
      }
      if (take) {
        const uint64_t at = (f.npacked + 3) & ~3ull;
        int rc = f.room(3, at + nb + 8, f.st->packed_cap);
        if (rc) return rc;
        if (at / 4 > 0xFFFFFFFFull || base > 0x7FFFFFFFull) {
          set_error("nvt_pq_decode_str_chunk: more than 16 GiB of packed indices in one partition");
          return NVT_EUNSUPPORTED;
        }
        memset(f.st->packed + f.npacked, 0, at - f.npacked);
        memcpy(f.st->packed + at, r.p, nb);
        f.npacked = at + nb;
        if ((rc = f.run(NVT_PQ_RUN_PACKED, bw, (uint32_t)base, (uint32_t)(at / 4), take))) return rc;
      }
      r.skip_bytes(groups * bw < avail ? groups * bw : avail);   // (a writer may cut the padding)
      done += take;
    } else {   // RLE: (head >> 1) times the value in the next ceil(bw / 8) bytes
      uint64_t n = head >> 1;
      const unsigned vb = (bw + 7) / 8;
      if (avail < vb) {
        set_error("nvt_pq_decode_str_chunk: a repeat run past its page");
        return NVT_EINVAL;
      }
      uint64_t idx = 0;
      memcpy(&idx, r.p, vb);
      r.p += vb;
      idx &= mask;
      if (n > count - done) n = count - done;
      const int rc = f.run(NVT_PQ_RUN_REPEAT, 0, idx < ndict ? (uint32_t)(base + idx) : kBadId, 0, n);
      if (rc) return rc;
      done += n;
    }
  }
  return NVT_OK;
}

// the value sink: a string chunk keeps nothing between pages -- the dictionary's values are appended
// to the entries at once, so every page is inflated at the bottom of the scratch
struct StrValues : ValueSink {
  StrFill f;
  uint64_t base = 0, ndict = 0;   // the chunk's dictionary: entries [base, base + ndict)
  explicit StrValues(const StrFill &f_) : f(f_) {}
  bool takes_dictionary(const PageHead &) const { return true; }
  int dictionary(const char *who, const PageHead &h, const uint8_t *d) {
    // every value holds a 4-byte length: compared by division, a count of 2^61 must not wrap
    if (h.dict_values < 0 || (uint64_t)h.dict_values > (uint64_t)h.uncompressed / 4) {
      set_error("%s: dictionary page holds fewer values than it says", who);
      return NVT_EINVAL;
    }
    base = f.entries;
    ndict = (uint64_t)h.dict_values;
    return str_append_plain(f, d, d + h.uncompressed, ndict);
  }
  int accepts(const char *who, const PageHead &h, bool have_dict) const { return plain_or_dictionary(who, h, have_dict); }
  int page(const char *who, const PageHead &h, const uint8_t *q, const uint8_t *pend, uint64_t pvalid) {
    int rc;
    if (by_dictionary(h)) {
      rc = str_index_runs(f, q, pend, pvalid, base, ndict);
    } else {
      const uint64_t first = f.entries;
      rc = str_append_plain(f, q, pend, pvalid);
      if (!rc) rc = f.run(NVT_PQ_RUN_SEQUENCE, 0, (uint32_t)first, 0, pvalid);
    }
    if (rc) return rc;
    if (f.entries > 0x7FFFFFFEull || f.nvalues > 0x7FFFFFFEull) {
      set_error("%s: more than 2^31 - 2 entries or values in one partition", who);
      return NVT_EUNSUPPORTED;
    }
    return NVT_OK;
  }
};

}  // namespace
}  // namespace nvt

using namespace nvt;

extern "C" int nvt_pq_decode_str_chunk(const uint8_t *chunk, uint64_t chunk_bytes, int codec, int max_def_level,
                                       uint64_t expect_rows, uint8_t *valid_out, uint64_t valid_bit_offset,
                                       nvt_pq_str_stage *stage, uint8_t *scratch, uint64_t scratch_bytes,
                                       uint64_t *need) {
  NVT_CHECK_ARG(chunk && stage && need, "null pointer");
  NVT_CHECK_ARG(stage->offsets && stage->chars && stage->runs && stage->packed, "null staging buffer");
  const PageWalk w{__func__, chunk, chunk_bytes, codec, expect_rows, scratch, scratch_bytes};
  FlatLevels lv{valid_out, valid_bit_offset, max_def_level};
  NVT_CHECK_ARG(lv.bad_args() == nullptr, lv.bad_args());
  NVT_CHECK_ARG(stage->runs_cap >= 1 && stage->nruns < stage->runs_cap && stage->packed_cap >= 8 &&
                    stage->npacked <= stage->packed_cap - 8 && stage->entries <= stage->entries_cap &&
                    stage->nchars <= stage->chars_cap && (stage->chars_cap & 3) == 0,
                "the stage's fill state does not fit its capacities");
  StrValues vs(StrFill{stage, stage->entries, stage->nchars, stage->nruns, stage->npacked, stage->nvalues, need});
  need[0] = need[1] = need[2] = need[3] = 0;
  if (vs.f.entries == 0) stage->offsets[0] = 0;
  const int rc = walk_pages(w, lv, vs);
  if (rc) return rc;
  // the closing record (the next chunk writes over it) and the 8 readable bytes behind the packed runs
  const StrFill &f = vs.f;
  uint32_t *close = stage->runs + 4 * f.nruns;
  close[0] = (uint32_t)f.nvalues;
  close[1] = NVT_PQ_RUN_END;
  close[2] = close[3] = 0;
  memset(stage->packed + f.npacked, 0, 8);
  memset(stage->chars + f.nchars, 0, ((f.nchars + 3) & ~3ull) - f.nchars);
  stage->entries = f.entries;
  stage->nchars = f.nchars;
  stage->nruns = f.nruns;
  stage->npacked = f.npacked;
  stage->nvalues = f.nvalues;
  return NVT_OK;
}
