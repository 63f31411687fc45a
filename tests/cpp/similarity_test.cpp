// C++ similarity-hash test (runs on a GPU box): ricepp_amd::similarity_hashes
// against expected digests for a set of files, given as argv[1] (the files'
// bytes back to back) and argv[2] (one line per file: size, the nilsimsa
// hexdigest, the 32-bit similarity value as 8 hex digits).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

#include "ricepp_amd.h"
#include "ricepp_amd.hpp"

static int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

static std::vector<uint8_t> read_file(char const* path) {
  std::vector<uint8_t> v;
  if (FILE* f = std::fopen(path, "rb")) {
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: similarity_test <files' bytes> <table>\n");
    return 2;
  }
  const std::vector<uint8_t> bytes = read_file(argv[1]);
  std::vector<size_t> sizes;
  std::vector<std::string> nil, sim;
  if (FILE* f = std::fopen(argv[2], "r")) {
    unsigned long long size;
    char a[80], b[16];
    while (std::fscanf(f, "%llu %79s %15s", &size, a, b) == 3) {
      sizes.push_back(size);
      nil.emplace_back(a);
      sim.emplace_back(b);
    }
    std::fclose(f);
  }
  const size_t n = sizes.size();
  CHECK(n > 0);
  std::vector<std::span<uint8_t const>> files;
  size_t at = 0, largest = 0;
  for (size_t b = 0; b < n && at + sizes[b] <= bytes.size(); at += sizes[b++]) {
    files.emplace_back(bytes.data() + at, sizes[b]);
    largest = sizes[b] > largest ? sizes[b] : largest;
  }
  CHECK(files.size() == n && at == bytes.size());
  if (failures) return 1;

  const ricepp_amd::similarity_digests rn = ricepp_amd::similarity_hashes(files);  // (nilsimsa, the default order's)
  CHECK(rn.digest_size == 32 && rn.digests.size() == 32 * n && rn.has == std::vector<uint8_t>(n, 1));
  const ricepp_amd::similarity_digests rs = ricepp_amd::similarity_hashes(files, "similarity");
  CHECK(rs.digest_size == 4 && rs.digests.size() == 4 * n && rs.has == std::vector<uint8_t>(n, 1));
  for (size_t b = 0; b < n && !failures; ++b) {
    CHECK(rn.hexdigest(b) == nil[b]);
    CHECK(rs.hexdigest(b) == sim[b]);
    // the host restatement agrees
    std::vector<uint8_t> state(rpp_similarity_state_bytes(RPP_SIMILARITY_NILSIMSA));  // zero = initial
    uint8_t out[32];
    CHECK(rpp_similarity_host_update(RPP_SIMILARITY_NILSIMSA, state.data(), files[b].data(), files[b].size()) == RPP_OK);
    CHECK(rpp_similarity_host_finalize(RPP_SIMILARITY_NILSIMSA, state.data(), out) == RPP_OK);
    CHECK(std::memcmp(out, rn.digests.data() + 32 * b, 32) == 0);
  }

  // max_size: a file of exactly max_size is hashed, a larger one is not (zero digest bytes)
  if (largest > 0) {
    const ricepp_amd::similarity_digests r = ricepp_amd::similarity_hashes(files, "nilsimsa", largest - 1);
    for (size_t b = 0; b < n && r.has.size() == n; ++b) {
      CHECK(r.has[b] == (sizes[b] <= largest - 1 ? 1 : 0));
      if (r.has[b])
        CHECK(r.hexdigest(b) == nil[b]);
      else
        CHECK(r.hexdigest(b) == std::string(64, '0'));
    }
    CHECK(ricepp_amd::similarity_hashes(files, "nilsimsa", largest).has == std::vector<uint8_t>(n, 1));
  }

  // the reference's own vector (test/nilsimsa_test.cpp)
  {
    char const* text = "abcdefgh";
    std::vector<std::span<uint8_t const>> one{{reinterpret_cast<uint8_t const*>(text), 8}};
    CHECK(ricepp_amd::similarity_hashes(one).hexdigest(0) ==
          "14c8118000000000030800000004042004189020001308014088003280000078");
    one[0] = {};
    CHECK(ricepp_amd::similarity_hashes(one, "similarity").hexdigest(0) == "00010203");
  }
  CHECK(ricepp_amd::similarity_hashes({}).digests.empty());
  bool thrown = false;
  try {
    (void)ricepp_amd::similarity_hashes(files, "md5");
  } catch (std::runtime_error const& e) {
    thrown = std::strstr(e.what(), "md5") != nullptr;
  }
  CHECK(thrown);

  ricepp_amd::shutdown_facade();
  if (failures) {
    std::fprintf(stderr, "similarity_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("similarity_test: OK\n");
  return 0;
}
