// mzxml_check.cpp -- the two value rules of csrc/mzxml_value.hpp as a stand-alone host program, for a sanitizer build
// (tests/test_mzxml_cpu.py compiles it with -fsanitize=address,undefined and runs it over a corpus it writes).
//
//   mzxml_check CORPUS
//
// CORPUS: records of  u8 kind | ...
//   kind 0, a retentionTime value:  u8 expect_deferred | u32 n | n bytes | 8 bytes: the minutes as a double's bits
//   kind 1, a decoded stream:       u8 precision (32, 64) | u32 n_peaks | n_peaks * 2 * precision / 8 bytes |
//                                   n_peaks float32 m/z | n_peaks float32 intensities (compared as bytes)
// Every buffer is allocated at its exact size, so that a read or write outside it is the sanitizer's to find. Exit
// status 0: every verdict and every byte as expected; 1: a mismatch (printed); 2: usage or a broken corpus.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mzxml_value.hpp"

static bool get32(const std::vector<uint8_t> &d, size_t &p, uint32_t *v) {
  if (d.size() - p < 4) return false;
  std::memcpy(v, d.data() + p, 4);
  p += 4;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 2;
  std::vector<uint8_t> d;
  uint8_t chunk[1 << 16];
  for (size_t r; (r = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) d.insert(d.end(), chunk, chunk + r);
  std::fclose(f);
  size_t p = 0, n_rec = 0, n_bad = 0;
  while (p < d.size()) {
    if (d.size() - p < 2) return 2;
    const int kind = d[p], arg = d[p + 1];
    p += 2;
    uint32_t n;
    if (!get32(d, p, &n)) return 2;
    bool same;
    if (kind == 0) {
      if (d.size() - p < (size_t)n + 8) return 2;
      std::unique_ptr<char[]> s(new char[n]);
      std::memcpy(s.get(), d.data() + p, n);
      double got = 0.0;
      const int rc = asl::mzx_duration(s.get(), (int)n, &got);
      same = rc == 1 ? arg == 1 : arg == 0 && std::memcmp(&got, d.data() + p + n, 8) == 0;
      if (!same) std::printf("record %zu: duration rc = %d, %.17g\n", n_rec, rc, got);
      p += (size_t)n + 8;
    } else if (kind == 1 && (arg == 32 || arg == 64)) {
      const size_t raw_n = (size_t)n * 2 * (arg / 8);
      if (d.size() - p < raw_n + (size_t)n * 8) return 2;
      std::unique_ptr<uint8_t[]> raw(new uint8_t[raw_n]);
      std::unique_ptr<float[]> mz(new float[n]), it(new float[n]);
      std::memcpy(raw.get(), d.data() + p, raw_n);
      for (uint32_t i = 0; i < n; ++i) asl::mzx_pair(raw.get(), i, (uint32_t)arg / 8u, mz.get() + i, it.get() + i);
      same = std::memcmp(mz.get(), d.data() + p + raw_n, (size_t)n * 4) == 0 &&
             std::memcmp(it.get(), d.data() + p + raw_n + (size_t)n * 4, (size_t)n * 4) == 0;
      if (!same) std::printf("record %zu: %u pairs of %d bits differ\n", n_rec, n, arg);
      p += raw_n + (size_t)n * 8;
    } else {
      return 2;
    }
    if (!same) ++n_bad;
    ++n_rec;
  }
  std::printf("%zu records, %zu mismatches\n", n_rec, n_bad);
  return n_bad == 0 ? 0 : 1;
}
