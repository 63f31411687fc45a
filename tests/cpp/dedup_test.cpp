// C++ duplicate-file test (runs on a GPU box): ricepp_amd::find_duplicates
// against the scanner's decision for a set of files, given as argv[1] (the
// files' bytes back to back) and argv[2] (one line per file: size, first,
// hashed, the XXH3-128 in DwarFS's byte order as hex or "-").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

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

static std::string hex(uint8_t const* p, size_t n) {
  static char const digits[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += digits[p[i] >> 4];
    s += digits[p[i] & 15];
  }
  return s;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: dedup_test <files' bytes> <table>\n");
    return 2;
  }
  const std::vector<uint8_t> bytes = read_file(argv[1]);
  std::vector<size_t> sizes;
  std::vector<uint32_t> first;
  std::vector<int> hashed;
  std::vector<std::string> digest;
  if (FILE* f = std::fopen(argv[2], "r")) {
    unsigned long long size;
    unsigned fi;
    int h;
    char d[80];
    while (std::fscanf(f, "%llu %u %d %79s", &size, &fi, &h, d) == 4) {
      sizes.push_back(size);
      first.push_back(fi);
      hashed.push_back(h);
      digest.emplace_back(d);
    }
    std::fclose(f);
  }
  const size_t n = sizes.size();
  CHECK(n > 0);
  std::vector<std::span<uint8_t const>> files;
  size_t at = 0;
  for (size_t b = 0; b < n && at + sizes[b] <= bytes.size(); at += sizes[b++])
    files.emplace_back(bytes.data() + at, sizes[b]);
  CHECK(files.size() == n && at == bytes.size());
  if (failures) return 1;

  const ricepp_amd::duplicate_files res = ricepp_amd::find_duplicates(files);  // (xxh3-128, the writer's default)
  CHECK(res.digest_size == 16);
  CHECK(res.first.size() == n && res.hashed.size() == n && res.digests.size() == 16 * n);
  for (size_t b = 0; b < n && res.first.size() == n; ++b) {
    CHECK(res.first[b] == first[b]);
    CHECK(res.hashed[b] == hashed[b]);
    if (hashed[b])
      CHECK(hex(res.digests.data() + 16 * b, 16) == digest[b]);
    else
      CHECK(hex(res.digests.data() + 16 * b, 16) == std::string(32, '0'));
  }

  // the other algorithms decide the same; their digests agree with the decision
  for (auto [algo, width] : {std::pair<char const*, size_t>{"xxh3-64", 8}, {"sha512-256", 32}}) {
    const ricepp_amd::duplicate_files r = ricepp_amd::find_duplicates(files, algo);
    CHECK(r.digest_size == width && r.digests.size() == width * n);
    CHECK(r.first == res.first && r.hashed == res.hashed);
    for (size_t b = 0; b < n && r.first.size() == n; ++b)
      if (r.hashed[b])
        CHECK(std::memcmp(r.digests.data() + width * b, r.digests.data() + width * r.first[b], width) == 0);
  }

  // the reference's own vector (test/checksum_test.cpp:75): a file is hashed once another shares its size
  {
    char const* hello = "Hello, World!";
    char const* other = "Hello, World?";
    std::vector<std::span<uint8_t const>> two{{reinterpret_cast<uint8_t const*>(hello), 13},
                                              {reinterpret_cast<uint8_t const*>(other), 13}};
    const ricepp_amd::duplicate_files r = ricepp_amd::find_duplicates(two, "xxh3-128");
    CHECK(r.hashed == std::vector<uint8_t>({1, 1}) && r.first == std::vector<uint32_t>({0, 1}));
    CHECK(hex(r.digests.data(), 16) == "9553d72c8403db7750dd474484f21d53");
    two[1] = two[0];
    CHECK(ricepp_amd::find_duplicates(two).first == std::vector<uint32_t>({0, 0}));
  }
  CHECK(ricepp_amd::find_duplicates({}).first.empty());
  bool thrown = false;
  try {
    (void)ricepp_amd::find_duplicates(files, "md5");
  } catch (std::runtime_error const& e) {
    thrown = std::strstr(e.what(), "md5") != nullptr;
  }
  CHECK(thrown);

  ricepp_amd::shutdown_facade();
  if (failures) {
    std::fprintf(stderr, "dedup_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("dedup_test: OK\n");
  return 0;
}
