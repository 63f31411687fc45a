// C++ section test (runs on a GPU box): ricepp_amd::make_sections and
// check_sections against sections written by the reference (an image file of
// them is given as argv[1]) and one round trip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <span>
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
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: section_test <image of reference sections>\n");
    return 2;
  }
  const std::vector<uint8_t> ref = read_file(argv[1]);
  CHECK(ref.size() > 128);

  // the reference's sections verify at both levels, and are reproduced byte
  // for byte from their payload, number, type and compression
  for (int level : {1, 2}) {
    const std::vector<int> st = ricepp_amd::check_sections(ref, level);
    CHECK(st.size() == 2);
    for (int s : st) CHECK(s == RPP_OK);
  }
  size_t nsec = 0;
  for (size_t at = 0; at + 64 <= ref.size(); ++nsec) {
    rpp_section_header h;
    CHECK(rpp_parse_section_header(ref.data() + at, &h) == RPP_OK);
    if (h.length > ref.size() - at - 64) break;
    std::vector<std::vector<uint8_t>> payload(1);
    payload[0].assign(ref.begin() + at + 64, ref.begin() + at + 64 + h.length);
    const std::vector<uint8_t> made = ricepp_amd::make_sections(payload, h.number, h.type, h.compression);
    CHECK(made.size() == 64 + h.length);
    // (byte 7 is the minor version, covered by neither checksum: the images
    // of the reference's tests were written at earlier minor versions)
    CHECK(made.size() == 64 + h.length && std::memcmp(made.data(), ref.data() + at, 7) == 0 && made[7] == 5 &&
          std::memcmp(made.data() + 8, ref.data() + at + 8, made.size() - 8) == 0);
    at += 64 + h.length;
  }
  CHECK(nsec == 2);

  // round trip: odd sizes (every class of the short hash, several 1 KiB blocks,
  // an empty payload), byte-packed
  std::mt19937 rng(7);
  std::vector<std::vector<uint8_t>> payloads;
  for (size_t n : {0u, 1u, 5u, 13u, 100u, 200u, 241u, 1024u, 1025u, 70001u}) {
    std::vector<uint8_t> p(n);
    for (auto& b : p) b = (uint8_t)rng();
    payloads.push_back(std::move(p));
  }
  const std::vector<uint8_t> image = ricepp_amd::make_sections(payloads, 7, 0, 7);
  size_t at = 0;
  for (size_t b = 0; b < payloads.size(); ++b) {
    rpp_section_header h;
    CHECK(at + 64 <= image.size() && rpp_parse_section_header(image.data() + at, &h) == RPP_OK);
    CHECK(h.number == 7 + b && h.type == 0 && h.compression == 7 && h.length == payloads[b].size());
    CHECK(h.major == 2 && h.minor == 5);
    CHECK(std::memcmp(image.data() + at + 64, payloads[b].data(), payloads[b].size()) == 0);
    at += 64 + payloads[b].size();
  }
  CHECK(at == image.size());
  for (int level : {1, 2}) {
    const std::vector<int> st = ricepp_amd::check_sections(image, level);
    CHECK(st.size() == payloads.size());
    for (int s : st) CHECK(s == RPP_OK);
  }
  {
    std::vector<uint8_t> bad = image;
    bad.back() ^= 0x40;  // the last section's last payload byte
    std::vector<int> st = ricepp_amd::check_sections(bad, 1);
    CHECK(st.size() == payloads.size() && st.back() == RPP_CHECKSUM_MISMATCH && st.front() == RPP_OK);
    bad = image;
    bad[8] ^= 1;  // the first section's SHA
    CHECK(ricepp_amd::check_sections(bad, 1).front() == RPP_OK);
    CHECK(ricepp_amd::check_sections(bad, 2).front() == RPP_CHECKSUM_MISMATCH);
    bad = image;
    bad.pop_back();
    st = ricepp_amd::check_sections(bad, 1);
    CHECK(st.size() == payloads.size() && st.back() == RPP_TRUNCATED_INPUT);
    bad = image;
    bad[0] = 'X';
    st = ricepp_amd::check_sections(bad, 2);
    CHECK(st.size() == 1 && st[0] == RPP_INVALID_ARGUMENT);
  }
  CHECK(ricepp_amd::make_sections(std::vector<std::vector<uint8_t>>{}, 0, 0, 0).empty());
  CHECK(ricepp_amd::check_sections({}, 1).empty());

  ricepp_amd::shutdown_facade();
  if (failures) {
    std::fprintf(stderr, "section_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("section_test: OK\n");
  return 0;
}
