// C++ test of the host encoders under the search word
// (rpp_lz4_host_encode_search in dwarfs_amd/csrc/lz4_host.cpp,
// rpp_zstd_host_encode_search in zstd_encode_host.cpp), built by build_search.sh
// with AddressSanitizer and UBSan into a program of its own: no GPU, no
// library, nothing loaded into another process.  argv[1] is a file of records
// written by tests/test_search_host.py:
//   int64 n, then per search word (0, 1, 2, 4, 8, 0x101, 0x102, 0x104, 0x108)
//   the bytes of the LZ4 block and of the zstd frame under options 3; then the
//   input (n bytes)
// Every input is encoded under every word into a heap block of exactly the
// bound's bytes, the result copied into a block of exactly its size and decoded
// into a block of exactly n bytes, so a byte read or written outside them stops
// the program.  The results must have the stated sizes and decode to the input;
// word 0 must give the bytes of the calls without a word, word 1 the bytes of
// word 0, and an invalid word must be refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) {                                                                                               \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (record %ld, search %#x)\n", __FILE__, __LINE__, #cond, record, \
                   search);                                                                                      \
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

static const uint32_t kWords[9] = {0,
                                   1,
                                   2,
                                   4,
                                   8,
                                   1 | RPP_SEARCH_LAZY,
                                   2 | RPP_SEARCH_LAZY,
                                   4 | RPP_SEARCH_LAZY,
                                   8 | RPP_SEARCH_LAZY};
static const uint32_t kInvalid[7] = {3, 5, 16, RPP_SEARCH_LAZY, 0x200u | 2, 0x1000u | 8, 1u << 31};

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: search_test <vectors>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  long record = 0;
  int64_t head[19];
  while (std::fread(head, sizeof head, 1, f) == 1) {
    const uint64_t n = uint64_t(head[0]);
    std::vector<uint8_t> a(static_cast<size_t>(n));
    if (!a.empty() && std::fread(a.data(), a.size(), 1, f) != 1) return 2;
    const uint64_t lcap = rpp_lz4_bound(n), zcap = rpp_zstd_bound(n);
    Exact in{a.size(), a.data()};
    std::vector<uint8_t> lz4_0, zstd_0;
    for (int w = 0; w < 9; ++w) {
      const uint32_t search = kWords[w];
      uint64_t size = 0;
      uint32_t flag = 7;
      {  // LZ4
        Exact out{static_cast<size_t>(lcap)};
        CHECK(rpp_lz4_host_encode_search(in.p, n, search, out.p, lcap - 1, &size, &flag) == RPP_OUTPUT_TOO_SMALL);
        CHECK(rpp_lz4_host_encode_search(in.p, n, search, out.p, lcap, &size, &flag) == RPP_OK);
        CHECK(size == uint64_t(head[1 + 2 * w]) && size <= lcap && flag == (4 + size >= n ? 1u : 0u));
        Exact block{static_cast<size_t>(size), out.p}, back{static_cast<size_t>(n)};
        CHECK(rpp_lz4_host_decode(block.p, size, back.p, n) == RPP_OK);
        CHECK(n == 0 || std::memcmp(back.p, a.data(), size_t(n)) == 0);
        if (w == 0) {
          lz4_0.assign(block.p, block.p + size);
          Exact old{static_cast<size_t>(lcap)};
          uint64_t old_size = 0;
          CHECK(rpp_lz4_host_encode(in.p, n, old.p, lcap, &old_size, nullptr) == RPP_OK);
          CHECK(old_size == size && std::memcmp(old.p, block.p, size_t(size)) == 0);
        }
        if (w == 1) CHECK(size == lz4_0.size() && std::memcmp(lz4_0.data(), block.p, size_t(size)) == 0);
      }
      {  // Zstandard, options 3
        Exact out{static_cast<size_t>(zcap)};
        CHECK(rpp_zstd_host_encode_search(in.p, n, 3, search, out.p, zcap - 1, &size, &flag) == RPP_OUTPUT_TOO_SMALL);
        CHECK(rpp_zstd_host_encode_search(in.p, n, 4, search, out.p, zcap, &size, &flag) == RPP_INVALID_ARGUMENT);
        CHECK(rpp_zstd_host_encode_search(in.p, n, 3, search, out.p, zcap, &size, &flag) == RPP_OK);
        CHECK(size == uint64_t(head[2 + 2 * w]) && size <= zcap && flag == (size >= n ? 1u : 0u));
        Exact frame{static_cast<size_t>(size), out.p}, back{static_cast<size_t>(n)};
        CHECK(rpp_zstd_host_decode(frame.p, size, back.p, n) == RPP_OK);
        CHECK(n == 0 || std::memcmp(back.p, a.data(), size_t(n)) == 0);
        if (w == 0) {
          zstd_0.assign(frame.p, frame.p + size);
          Exact old{static_cast<size_t>(zcap)};
          uint64_t old_size = 0;
          CHECK(rpp_zstd_host_encode_opt(in.p, n, 3, old.p, zcap, &old_size, nullptr) == RPP_OK);
          CHECK(old_size == size && std::memcmp(old.p, frame.p, size_t(size)) == 0);
        }
        if (w == 1) CHECK(size == zstd_0.size() && std::memcmp(zstd_0.data(), frame.p, size_t(size)) == 0);
      }
    }
    for (const uint32_t search : kInvalid) {
      Exact out{static_cast<size_t>(zcap > lcap ? zcap : lcap)};
      uint64_t size = 0;
      CHECK(rpp_lz4_host_encode_search(in.p, n, search, out.p, lcap, &size, nullptr) == RPP_INVALID_ARGUMENT);
      CHECK(rpp_zstd_host_encode_search(in.p, n, 0, search, out.p, zcap, &size, nullptr) == RPP_INVALID_ARGUMENT);
    }
    ++record;
  }
  std::fclose(f);
  const uint32_t search = 0;
  CHECK(record > 0);
  if (failures) {
    std::fprintf(stderr, "search_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("search_test: OK (%ld records)\n", record);
  return 0;
}
