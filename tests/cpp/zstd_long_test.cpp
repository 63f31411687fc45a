// C++ test of the Zstandard host encoder's `long` word
// (rpp_zstd_host_encode_long, dwarfs_amd/csrc/zstd_long_host.cpp), built by
// build_zstd_long.sh with AddressSanitizer and UBSan into a program of its own:
// no GPU, no library, nothing loaded into another process.  First every size
// from 0 to 200, as random bytes, as zeros and as a block whose second half
// repeats its first; then argv[1], a file of records written by
// tests/test_zstd_long_host.py:
//   int64 n, frame_bytes (options 3, search 0, long 1); then the input (n bytes)
// Every input is encoded into a heap block of exactly rpp_zstd_bound(n) bytes,
// the frame copied into a block of exactly its size and decoded into a block of
// exactly n bytes, so a byte read or written outside them stops the program.
// long 0 must give the bytes of rpp_zstd_host_encode_search, a long word above 1
// must be refused, and the debug export must state as many sequences as fit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) {                                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (record %ld, n %llu)\n", __FILE__, __LINE__, #cond, record, \
                   (unsigned long long)n);                                                                       \
      ++failures;                                                                                                \
    }                                                                                                            \
  } while (0)

// a heap block of exactly n bytes (n == 0: a one-byte block that is never offered as more than 0 bytes)
struct Exact {
  uint8_t* p;
  explicit Exact(size_t n, const uint8_t* from = nullptr) : p(static_cast<uint8_t*>(std::malloc(n ? n : 1))) {
    if (from && n) std::memcpy(p, from, n);
  }
  ~Exact() { std::free(p); }
};

// encode with (options, search, long 1), decode, compare; the frame's size
static uint64_t round_trip(const std::vector<uint8_t>& a, uint32_t options, uint32_t search, long record) {
  const uint64_t n = a.size(), cap = rpp_zstd_bound(n);
  Exact in{a.size(), a.data()}, out{static_cast<size_t>(cap)};
  uint64_t size = 0;
  uint32_t flag = 7;
  CHECK(rpp_zstd_host_encode_long(in.p, n, options, search, 1, out.p, cap - 1, &size, &flag) == RPP_OUTPUT_TOO_SMALL);
  CHECK(rpp_zstd_host_encode_long(in.p, n, options, search, 2, out.p, cap, &size, &flag) == RPP_INVALID_ARGUMENT);
  CHECK(rpp_zstd_host_encode_long(in.p, n, options, search, 1, out.p, cap, &size, &flag) == RPP_OK);
  CHECK(size <= cap && flag == (size >= n ? 1u : 0u));
  Exact frame{static_cast<size_t>(size), out.p}, back{static_cast<size_t>(n)};
  uint64_t content = 0;
  uint32_t flags = 0;
  CHECK(rpp_zstd_frame_info(frame.p, size, &content, nullptr, &flags) > 0);
  CHECK((flags & RPP_ZSTD_FLAG_CONTENT_SIZE) && content == n);
  CHECK(rpp_zstd_host_decode(frame.p, size, back.p, n) == RPP_OK);
  CHECK(n == 0 || std::memcmp(back.p, a.data(), size_t(n)) == 0);
  // long 0 is the search call
  Exact old{static_cast<size_t>(cap)}, same{static_cast<size_t>(cap)};
  uint64_t old_size = 0, same_size = 1;
  CHECK(rpp_zstd_host_encode_search(in.p, n, options, search, old.p, cap, &old_size, nullptr) == RPP_OK);
  CHECK(rpp_zstd_host_encode_long(in.p, n, options, search, 0, same.p, cap, &same_size, nullptr) == RPP_OK);
  CHECK(old_size == same_size && std::memcmp(old.p, same.p, size_t(old_size)) == 0);
  // the debug export: the count first, then exactly that many triples
  uint64_t count = 0;
  const int st = rpp_zstd_host_long_sequences(in.p, n, search, 1, nullptr, 0, &count);
  CHECK(st == (count ? RPP_OUTPUT_TOO_SMALL : RPP_OK));
  Exact triples{static_cast<size_t>(12 * count)};
  CHECK(rpp_zstd_host_long_sequences(in.p, n, search, 1, reinterpret_cast<uint32_t*>(triples.p), count, &count) ==
        RPP_OK);
  return size;
}

int main(int argc, char** argv) {
  long record = -1;
  uint32_t seed = 12345;
  for (uint64_t n = 0; n <= 200; ++n) {
    std::vector<uint8_t> random(n), zeros(n, 0), twice(n);
    for (auto& b : random) b = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
    for (uint64_t i = 0; i < n; ++i) twice[i] = random[i % (n / 2 ? n / 2 : 1)];
    for (uint32_t options : {0u, 3u}) {
      round_trip(random, options, 0, record);
      round_trip(zeros, options, 0, record);
      round_trip(twice, options, 8u | RPP_SEARCH_LAZY, record);
    }
  }
  record = 0;
  uint64_t n = 0;
  if (argc >= 2) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[2];
    while (std::fread(head, sizeof head, 1, f) == 1) {
      n = uint64_t(head[0]);
      std::vector<uint8_t> a(static_cast<size_t>(n));
      if (!a.empty() && std::fread(a.data(), a.size(), 1, f) != 1) return 2;
      CHECK(round_trip(a, 3, 0, record) == uint64_t(head[1]));
      round_trip(a, 0, 8u | RPP_SEARCH_LAZY, record);
      ++record;
    }
    std::fclose(f);
    CHECK(record > 0);
  }
  if (failures) {
    std::fprintf(stderr, "zstd_long_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("zstd_long_test: OK (%ld records)\n", record);
  return 0;
}
