// Host-only sanitizer harness of the parquet string decoder (nvt_pq_decode_str_chunk, the host C of
// nvtabular_amd/csrc/nvt_parquet.hip): decodes the string chunks of a file as they are, then a few
// thousand byte-mutated copies of each (fixed seed).  Every call must return NVT_OK or an error;
// AddressSanitizer / UBSan watch the reads of the chunk and the writes of the staging buffers, which
// are heap blocks of exactly the documented sizes.  Every chunk is decoded twice: into buffers sized
// generously from the footer, and from capacities of almost nothing, enlarged as the decoder asks
// (NVT_PQ_STR_GROW) -- both must end the same way.  Runs on the CPU: nothing here
// touches a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tools/pq_str_fuzz.cpp nvtabular_amd/csrc/nvt_parquet.hip nvtabular_amd/csrc/nvt_util.hip -ldl -o tools/pq_str_fuzz
//   tools/pq_str_fuzz FILE $(python tools/pq_str_fuzz_chunks.py FILE) [mutations per chunk, default 4000]
//
// A chunk is offset:size:codec:max_def:rows:raw_size (pq_str_fuzz_chunks.py prints them from the footer).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/nvt_hip.h"

struct Rng {  // xorshift64*: the same mutations on every run
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
  }
  uint64_t below(uint64_t n) { return next() % n; }
};

struct Stage {  // heap blocks of exactly the documented sizes
  std::vector<int64_t> offsets;
  std::vector<uint8_t> chars, packed;
  std::vector<uint32_t> runs;
  nvt_pq_str_stage st;
  Stage(uint64_t e, uint64_t c, uint64_t r, uint64_t p) : offsets(e + 1), chars(c), packed(p), runs(4 * r) {
    std::memset(&st, 0, sizeof st);
    bind();
  }
  void bind() {
    st.offsets = offsets.data();
    st.chars = chars.data();
    st.runs = runs.data();
    st.packed = packed.data();
    st.entries_cap = offsets.size() - 1;
    st.chars_cap = chars.size();
    st.runs_cap = runs.size() / 4;
    st.packed_cap = packed.size();
  }
  // fresh blocks (the old ones are freed: a pointer kept by the decoder would be a sanitizer report)
  void grow(const uint64_t need[4]) {   // (at least twice the old size: a chunk is decoded again after every grow)
    auto cap = [](uint64_t want, uint64_t old) { return want > 2 * old ? want : 2 * old; };
    if (need[0]) { std::vector<int64_t> n(cap(need[0], st.entries_cap) + 1); std::memcpy(n.data(), offsets.data(), (st.entries + 1) * 8); offsets.swap(n); }
    if (need[1]) { std::vector<uint8_t> n((cap(need[1], st.chars_cap) + 3) & ~3ull); std::memcpy(n.data(), chars.data(), st.nchars); chars.swap(n); }
    if (need[2]) { std::vector<uint32_t> n(4 * cap(need[2], st.runs_cap)); std::memcpy(n.data(), runs.data(), 16 * st.nruns); runs.swap(n); }
    if (need[3]) { std::vector<uint8_t> n(cap(need[3], st.packed_cap)); std::memcpy(n.data(), packed.data(), st.npacked); packed.swap(n); }
    bind();
  }
};

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s FILE offset:size:codec:max_def:rows:raw_size ... [mutations]\n", argv[0]);
    return 2;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  long mutations = 4000;
  Rng rng{0x9E3779B97F4A7C15ull};
  long calls = 0, ok = 0, einval = 0, eunsup = 0, grows = 0;
  for (int a = 2; a < argc; ++a) {
    unsigned long long off, size, codec, max_def, rows, raw;
    if (std::sscanf(argv[a], "%llu:%llu:%llu:%llu:%llu:%llu", &off, &size, &codec, &max_def, &rows, &raw) != 6) {
      mutations = std::atol(argv[a]);
      continue;
    }
    std::vector<uint8_t> chunk(size);
    if (std::fseek(f, (long)off, SEEK_SET) != 0 || std::fread(chunk.data(), 1, size, f) != size) {
      std::fprintf(stderr, "short read of chunk %s\n", argv[a]);
      return 2;
    }
    const uint64_t bound = 2 * (raw > size ? raw : size) + 64;   // what the chunk's bytes can spell out
    for (long it = 0; it <= mutations; ++it) {
      std::vector<uint8_t> buf(chunk);
      if (it) {
        const int k = 1 + (int)rng.below(3);
        for (int j = 0; j < k; ++j) {
          const uint64_t at = rng.below(2) ? rng.below(buf.size()) : rng.below(buf.size() < 64 ? buf.size() : 64);
          const uint64_t r = rng.below(10);
          buf[at] = r < 7 ? (uint8_t)rng.below(256) : (r < 9 ? 0xFF : 0x80);
        }
        if (rng.below(16) == 0) buf.resize(rng.below(buf.size()) + 1);   // and truncations
      }
      int rcs[2];
      uint64_t got[2][5];
      for (int pass = 0; pass < 2; ++pass) {
        Stage s = pass == 0 ? Stage(bound / 4 + 16, (bound + 3) & ~3ull, bound + 2, 4 * bound + 64) : Stage(1, 4, 1, 8);
        std::vector<uint8_t> valid((rows + 7) / 8 + 8), scratch(bound);
        uint64_t need[4];
        int rc;
        for (;;) {
          rc = nvt_pq_decode_str_chunk(buf.data(), buf.size(), (int)codec, (int)max_def, rows, valid.data(), 0, &s.st,
                                       scratch.data(), scratch.size(), need);
          ++calls;
          if (rc != NVT_PQ_STR_GROW) break;
          ++grows;
          s.grow(need);
        }
        rcs[pass] = rc;
        const uint64_t g[5] = {s.st.entries, s.st.nchars, s.st.nruns, s.st.npacked, s.st.nvalues};
        std::memcpy(got[pass], g, sizeof g);
        if (rc == NVT_OK && (s.st.nvalues > rows || s.st.runs[4 * s.st.nruns] != s.st.nvalues ||
                             (s.st.nruns && s.st.runs[4 * (s.st.nruns - 1)] >= s.st.nvalues))) {
          std::fprintf(stderr, "chunk %s, mutation %ld: NVT_OK with a broken run table\n", argv[a], it);
          return 1;
        }
      }
      if (rcs[0] != rcs[1] || (rcs[0] == NVT_OK && std::memcmp(got[0], got[1], sizeof got[0]) != 0)) {
        std::fprintf(stderr, "chunk %s, mutation %ld: rc %d with room, rc %d grown\n", argv[a], it, rcs[0], rcs[1]);
        return 1;
      }
      const int rc = rcs[0];
      if (rc == NVT_OK) ++ok;
      else if (rc == NVT_EINVAL) ++einval;
      else if (rc == NVT_EUNSUPPORTED) ++eunsup;
      else {
        std::fprintf(stderr, "chunk %s, mutation %ld: rc %d\n", argv[a], it, rc);
        return 1;
      }
      if (it == 0 && rc != NVT_OK) {
        std::fprintf(stderr, "chunk %s as it is: rc %d (%s)\n", argv[a], rc, nvt_last_error());
        return 1;
      }
    }
  }
  std::fclose(f);
  std::printf("%ld calls (%ld after a grow): %ld decoded, %ld NVT_EINVAL, %ld NVT_EUNSUPPORTED\n", calls, grows, ok, einval,
              eunsup);
  return 0;
}
