// Host-only sanitizer harness of the parquet list decoder (nvt_pq_decode_list_chunk, the host C of
// nvtabular_amd/csrc/nvt_parquet.hip): decodes the list chunks of a file as they are, then a few
// thousand byte-mutated copies of each (fixed seed).  Every call must return NVT_OK or an error;
// AddressSanitizer / UBSan watch the reads of the chunk and the writes of the outputs, which are
// heap blocks of exactly the documented sizes.  Runs on the CPU: nothing here touches a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tools/pq_list_fuzz.cpp nvtabular_amd/csrc/nvt_parquet.hip nvtabular_amd/csrc/nvt_util.hip -ldl -o pq_list_fuzz
//   ./pq_list_fuzz FILE $(python tools/pq_list_fuzz_chunks.py FILE) [mutations per chunk, default 4000]
//
// A chunk is offset:size:codec:type_size:leaf_level:max_def:slots:rows:raw_size (pq_list_fuzz_chunks.py
// prints them from the footer).
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

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s FILE offset:size:codec:type_size:leaf_level:max_def:slots:rows:raw_size ... [mutations]\n",
                 argv[0]);
    return 2;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  long mutations = 4000;
  Rng rng{0x9E3779B97F4A7C15ull};
  long calls = 0, ok = 0, einval = 0, eunsup = 0;
  for (int a = 2; a < argc; ++a) {
    unsigned long long off, size, codec, tsize, leaf_level, max_def, slots, rows, raw;
    if (std::sscanf(argv[a], "%llu:%llu:%llu:%llu:%llu:%llu:%llu:%llu:%llu", &off, &size, &codec, &tsize, &leaf_level,
                    &max_def, &slots, &rows, &raw) != 9) {
      mutations = std::atol(argv[a]);
      continue;
    }
    std::vector<uint8_t> chunk(size);
    if (std::fseek(f, (long)off, SEEK_SET) != 0 || std::fread(chunk.data(), 1, size, f) != size) {
      std::fprintf(stderr, "short read of chunk %s\n", argv[a]);
      return 2;
    }
    const unsigned width = max_def == 1 ? 1 : 2;
    const uint64_t sbytes = 2 * (raw > size ? raw : size) + 64;
    for (long it = 0; it <= mutations; ++it) {
      // fresh blocks of exactly the documented sizes: a byte outside is a sanitizer report
      std::vector<uint8_t> buf(chunk), rep(((slots + 63) / 64) * 8), def(((slots * width + 63) / 64) * 8),
          vals(slots * tsize), scratch(sbytes);
      if (it) {
        const int k = 1 + (int)rng.below(3);
        for (int j = 0; j < k; ++j) {
          const uint64_t at = rng.below(2) ? rng.below(buf.size()) : rng.below(buf.size() < 64 ? buf.size() : 64);
          const uint64_t r = rng.below(10);
          buf[at] = r < 7 ? (uint8_t)rng.below(256) : (r < 9 ? 0xFF : 0x80);
        }
        if (rng.below(16) == 0) buf.resize(rng.below(buf.size()) + 1);   // and truncations
      }
      uint64_t counts[4] = {0, 0, 0, 0};
      const int rc = nvt_pq_decode_list_chunk(buf.data(), buf.size(), (int)codec, (int)tsize, (int)leaf_level, (int)max_def,
                                              slots, rows, rep.data(), def.data(), 0, slots, vals.data(), vals.size(),
                                              scratch.data(), scratch.size(), counts);
      ++calls;
      if (rc == NVT_OK) {
        ++ok;
        if (counts[0] != slots || counts[1] != rows || counts[3] > counts[2] || counts[2] > slots) {
          std::fprintf(stderr, "chunk %s, mutation %ld: NVT_OK with counts %llu %llu %llu %llu\n", argv[a], it,
                       (unsigned long long)counts[0], (unsigned long long)counts[1], (unsigned long long)counts[2],
                       (unsigned long long)counts[3]);
          return 1;
        }
      } else if (rc == NVT_EINVAL) {
        ++einval;
      } else if (rc == NVT_EUNSUPPORTED) {
        ++eunsup;
      } else {
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
  std::printf("%ld calls: %ld decoded, %ld NVT_EINVAL, %ld NVT_EUNSUPPORTED\n", calls, ok, einval, eunsup);
  return 0;
}
