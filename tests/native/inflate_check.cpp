// inflate_check.cpp -- the decoder core of csrc/inflate.hpp as a stand-alone host program, for a sanitizer build
// (tests/test_mzml_cpu.py compiles it with -fsanitize=address,undefined and runs it over a corpus it writes).
//
//   inflate_check CORPUS
//
// CORPUS: records of  u8 zlib | u8 expect_error | u32 n | u32 cap | u32 n_want | n bytes base64 | n_want bytes.
// Every buffer is allocated at its exact size, so that a read or write outside it is the sanitizer's to find. Exit
// status 0: every verdict and every byte as expected; 1: a mismatch (printed); 2: usage or a broken corpus.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "inflate.hpp"

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
    const int zlib = d[p], expect_error = d[p + 1];
    p += 2;
    uint32_t n, cap, n_want;
    if (!get32(d, p, &n) || !get32(d, p, &cap) || !get32(d, p, &n_want)) return 2;
    if (d.size() - p < (size_t)n + n_want) return 2;
    std::unique_ptr<uint8_t[]> src(new uint8_t[n]), out(new uint8_t[cap]);
    const uint32_t tmp_cap = n / 4 * 3 + 3;
    std::unique_ptr<uint8_t[]> tmp(new uint8_t[tmp_cap]);
    std::memcpy(src.get(), d.data() + p, n);
    const uint8_t *want = d.data() + p + n;
    p += (size_t)n + n_want;
    asl::InfWork work;
    uint32_t n_out = 0;
    const int rc = asl::inf_array(src.get(), n, zlib, tmp.get(), tmp_cap, out.get(), cap, &n_out, &work);
    const bool same = rc != asl::INF_OK ? expect_error != 0
                                        : expect_error == 0 && n_out == n_want && std::memcmp(out.get(), want, n_want) == 0;
    if (!same) {
      std::printf("record %zu: rc = %d, %u bytes; expected %s, %u bytes\n", n_rec, rc, n_out,
                  expect_error ? "an error" : "success", n_want);
      ++n_bad;
    }
    ++n_rec;
  }
  std::printf("%zu records, %zu mismatches\n", n_rec, n_bad);
  return n_bad == 0 ? 0 : 1;
}
