// C++ test of the Zstandard host functions (dwarfs_amd/csrc/zstd_host.cpp), built
// by build_zstd.sh with AddressSanitizer and UBSan into a program of its own: no
// GPU, no library, nothing loaded into another process.  argv[1] is a file of
// records written by tests/test_zstd_host.py:
//   int64 n, expect, len_a, len_b; then a (len_a bytes), b (len_b bytes)
//   a is a frame offered n bytes: expect 1 -> RPP_OK and the output is b,
//   else RPP_CORRUPT_INPUT
// Every buffer is a heap block of exactly the size the contract names, so a
// byte read or written outside it stops the program.  Every frame is also walked
// by rpp_zstd_frame_info and rpp_zstd_count_blocks, and every cut of its first
// 24 bytes by all three.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (record %ld)\n", __FILE__, __LINE__, #cond, record); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// a heap block of exactly n bytes (n == 0: a one-byte block that is never offered as more than 0 bytes)
struct Exact {
  uint8_t* p;
  explicit Exact(size_t n, const uint8_t* from = nullptr) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))) {
    if (from && n) std::memcpy(p, from, n);
  }
  ~Exact() { std::free(p); }
};

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: zstd_test <vectors>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  long record = 0;
  int64_t head[4];
  while (std::fread(head, sizeof head, 1, f) == 1) {
    const int64_t n = head[0], expect = head[1];
    std::vector<uint8_t> a(static_cast<size_t>(head[2])), b(static_cast<size_t>(head[3]));
    if (!a.empty() && std::fread(a.data(), a.size(), 1, f) != 1) return 2;
    if (!b.empty() && std::fread(b.data(), b.size(), 1, f) != 1) return 2;
    Exact in{a.size(), a.data()}, out{static_cast<size_t>(n)};
    std::memset(out.p, 0xA5, size_t(n));
    const int st = rpp_zstd_host_decode(in.p, a.size(), out.p, uint64_t(n));
    if (expect) {
      CHECK(st == RPP_OK);
      CHECK(b.size() == size_t(n) && (n == 0 || std::memcmp(out.p, b.data(), size_t(n)) == 0));
      uint64_t content = 0, window = 0;
      uint32_t flags = 0;
      CHECK(rpp_zstd_frame_info(in.p, a.size(), &content, &window, &flags) > 0);
      CHECK(!(flags & RPP_ZSTD_FLAG_CONTENT_SIZE) || content == uint64_t(n));
      CHECK(rpp_zstd_count_blocks(in.p, a.size()) >= 1);
    } else {
      CHECK(st == RPP_CORRUPT_INPUT);
      (void)rpp_zstd_frame_info(in.p, a.size(), nullptr, nullptr, nullptr);
      (void)rpp_zstd_count_blocks(in.p, a.size());
    }
    for (size_t cut = 0; cut < a.size() && cut < 24; ++cut) {
      Exact part{cut, a.data()};
      (void)rpp_zstd_frame_info(part.p, cut, nullptr, nullptr, nullptr);
      CHECK(rpp_zstd_count_blocks(part.p, cut) == RPP_CORRUPT_INPUT || cut >= 9);
      CHECK(rpp_zstd_host_decode(part.p, cut, out.p, uint64_t(n)) != RPP_OK || cut >= 9);
    }
    ++record;
  }
  std::fclose(f);
  CHECK(record > 0);
  if (failures) {
    std::fprintf(stderr, "zstd_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("zstd_test: OK (%ld records)\n", record);
  return 0;
}
