// C++ test of the Zstandard host encoder's options word
// (rpp_zstd_host_encode_opt, dwarfs_amd/csrc/zstd_encode_host.cpp), built by
// build_zstd_encode_adaptive.sh with AddressSanitizer and UBSan into a program
// of its own: no GPU, no library, nothing loaded into another process.  argv[1]
// is a file of records written by tests/test_zstd_encode_adaptive_host.py:
//   int64 n, frame_bytes[4] (options 0 to 3); then the input (n bytes)
// Every input is encoded with each options word into a heap block of exactly
// rpp_zstd_bound(n) bytes, the frame copied into a block of exactly its size and
// decoded into a block of exactly n bytes, so a byte read or written outside
// them stops the program.  The frame must have the stated size, state n as its
// content size and decode to the input; options 0 must give the bytes of
// rpp_zstd_host_encode, and an unknown option bit must be refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (record %ld, options %u)\n", __FILE__, __LINE__, #cond, record, \
                   options);                                                \
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
    std::fprintf(stderr, "usage: zstd_encode_adaptive_test <vectors>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  long record = 0;
  int64_t head[5];
  while (std::fread(head, sizeof head, 1, f) == 1) {
    const uint64_t n = uint64_t(head[0]);
    std::vector<uint8_t> a(static_cast<size_t>(n));
    if (!a.empty() && std::fread(a.data(), a.size(), 1, f) != 1) return 2;
    const uint64_t cap = rpp_zstd_bound(n);
    Exact in{a.size(), a.data()};
    for (uint32_t options = 0; options < 4; ++options) {
      const uint64_t want = uint64_t(head[1 + options]);
      Exact out{static_cast<size_t>(cap)};
      uint64_t size = 0;
      uint32_t flag = 7;
      CHECK(rpp_zstd_host_encode_opt(in.p, n, options, out.p, cap - 1, &size, &flag) == RPP_OUTPUT_TOO_SMALL);
      CHECK(rpp_zstd_host_encode_opt(in.p, n, options | 4u, out.p, cap, &size, &flag) == RPP_INVALID_ARGUMENT);
      CHECK(rpp_zstd_host_encode_opt(in.p, n, options, out.p, cap, &size, &flag) == RPP_OK);
      CHECK(size == want && size <= cap && flag == (size >= n ? 1u : 0u));
      Exact frame{static_cast<size_t>(size), out.p}, back{static_cast<size_t>(n)};
      if (options == 0) {
        Exact old{static_cast<size_t>(cap)};
        uint64_t old_size = 0;
        CHECK(rpp_zstd_host_encode(in.p, n, old.p, cap, &old_size, nullptr) == RPP_OK);
        CHECK(old_size == size && std::memcmp(old.p, frame.p, size_t(size)) == 0);
      }
      uint64_t content = 0;
      uint32_t flags = 0;
      CHECK(rpp_zstd_frame_info(frame.p, size, &content, nullptr, &flags) > 0);
      CHECK((flags & RPP_ZSTD_FLAG_CONTENT_SIZE) && content == n);
      CHECK(rpp_zstd_host_decode(frame.p, size, back.p, n) == RPP_OK);
      CHECK(n == 0 || std::memcmp(back.p, a.data(), size_t(n)) == 0);
    }
    ++record;
  }
  std::fclose(f);
  const uint32_t options = 0;
  CHECK(record > 0);
  if (failures) {
    std::fprintf(stderr, "zstd_encode_adaptive_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("zstd_encode_adaptive_test: OK (%ld records)\n", record);
  return 0;
}
