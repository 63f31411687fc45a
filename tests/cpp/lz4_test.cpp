// C++ test of the LZ4 host functions (dwarfs_amd/csrc/lz4_host.cpp), built by
// build_lz4.sh with AddressSanitizer and UBSan into a program of its own: no
// GPU, no library, nothing loaded into another process.  argv[1] is a file of
// records written by tests/test_lz4_host.py:
//   int64 kind, n, expect, len_a, len_b; then a (len_a bytes), b (len_b bytes)
//   kind 0  a is a valid block of the n-byte input b: decode gives b
//   kind 1  a is a damaged block offered n bytes: expect 1 -> RPP_OK and b,
//           else RPP_OK or RPP_CORRUPT_INPUT
//   kind 2  a is an n-byte input: encode, check the bound, decode back
// Every buffer is a heap block of exactly the size the contract names, so a
// byte read or written outside it stops the program.
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
    std::fprintf(stderr, "usage: lz4_test <vectors>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  long record = 0;
  int64_t head[5];
  while (std::fread(head, sizeof head, 1, f) == 1) {
    const int64_t kind = head[0], n = head[1], expect = head[2];
    std::vector<uint8_t> a(static_cast<size_t>(head[3])), b(static_cast<size_t>(head[4]));
    if (!a.empty() && std::fread(a.data(), a.size(), 1, f) != 1) return 2;
    if (!b.empty() && std::fread(b.data(), b.size(), 1, f) != 1) return 2;
    if (kind == 0 || kind == 1) {
      Exact in{a.size(), a.data()}, out{static_cast<size_t>(n)};
      std::memset(out.p, 0xA5, size_t(n));
      const int st = rpp_lz4_host_decode(in.p, a.size(), out.p, uint64_t(n));
      if (kind == 0 || expect) {
        CHECK(st == RPP_OK);
        CHECK(b.size() == size_t(n) && (n == 0 || std::memcmp(out.p, b.data(), size_t(n)) == 0));
      } else {
        CHECK(st == RPP_OK || st == RPP_CORRUPT_INPUT);
      }
    } else {
      const uint64_t cap = rpp_lz4_bound(uint64_t(n));
      Exact in{a.size(), a.data()}, enc{cap}, back{static_cast<size_t>(n)};
      uint64_t size = 0;
      uint32_t flag = 2;
      CHECK(rpp_lz4_host_encode(in.p, uint64_t(n), enc.p, cap, &size, &flag) == RPP_OK);
      CHECK(size >= 1 && size <= cap && flag == (4 + size >= uint64_t(n) ? 1u : 0u));
      Exact tight{size, enc.p};  // decode from a block of exactly the encoded size
      CHECK(rpp_lz4_host_decode(tight.p, size, back.p, uint64_t(n)) == RPP_OK);
      CHECK(n == 0 || std::memcmp(back.p, a.data(), size_t(n)) == 0);
      if (size > 1) CHECK(rpp_lz4_host_decode(tight.p, size - 1, back.p, uint64_t(n)) == RPP_CORRUPT_INPUT);
    }
    ++record;
  }
  std::fclose(f);
  uint32_t v = 0;
  const uint8_t four[4] = {4, 3, 2, 1};
  uint8_t hdr[4];
  CHECK(rpp_lz4_frame_header(0x01020304u, hdr) == 4 && std::memcmp(hdr, four, 4) == 0);
  CHECK(rpp_lz4_parse_frame(four, 4, &v) == 4 && v == 0x01020304u);
  CHECK(rpp_lz4_parse_frame(four, 3, &v) == RPP_TRUNCATED_INPUT);
  CHECK(record > 0);
  if (failures) {
    std::fprintf(stderr, "lz4_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("lz4_test: OK (%ld records)\n", record);
  return 0;
}
