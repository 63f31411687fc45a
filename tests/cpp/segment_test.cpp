// C++ segmenter test (runs on a GPU box): ricepp_amd::segment_index and
// ricepp_amd::segment_scan against the host restatement, for a block (argv[1])
// and an extent (argv[2]) that holds verbatim pieces of it; argv[3..6] =
// window_bits, increment_shift, granularity, filter_bits; every further
// argument pos:off:frames names a piece planted at frame pos of the extent
// from frame off of the block.
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
  if (argc < 7) {
    std::fprintf(stderr, "usage: segment_test <block> <extent> <window_bits> <shift> <granularity> <filter_bits> [pos:off:frames ...]\n");
    return 2;
  }
  const std::vector<uint8_t> block = read_file(argv[1]), extent = read_file(argv[2]);
  ricepp_amd::segment_config cfg;
  cfg.window_bits = static_cast<uint32_t>(std::atoi(argv[3]));
  cfg.increment_shift = static_cast<uint32_t>(std::atoi(argv[4]));
  cfg.granularity = static_cast<uint32_t>(std::atoi(argv[5]));
  cfg.filter_bits = std::strtoull(argv[6], nullptr, 10);
  const rpp_segment_config c{cfg.window_bits, cfg.increment_shift, cfg.granularity, 0, cfg.filter_bits};
  CHECK(rpp_segment_check_config(&c) == RPP_OK);
  CHECK(!block.empty() && !extent.empty());
  if (failures) return 1;
  const uint32_t g = cfg.granularity, W = 1u << cfg.window_bits;
  const uint64_t bframes = block.size() / g, eframes = extent.size() / g, words = cfg.filter_bits / 64;

  // the index against the host restatement
  const ricepp_amd::segment_block_index idx = ricepp_amd::segment_index(block, cfg);
  const uint64_t slots = rpp_segment_index_slots(&c, bframes);
  CHECK(idx.hash.size() == slots && idx.offset.size() == slots && idx.entered.size() == slots && idx.filter.size() == words);
  std::vector<uint32_t> hh(slots), ho(slots);
  std::vector<uint8_t> he(slots);
  std::vector<uint64_t> bf(words), gf(words);
  CHECK(rpp_segment_host_index(&c, block.data(), bframes, hh.data(), ho.data(), he.data(), bf.data(), gf.data()) == RPP_OK);
  CHECK(idx.hash == hh && idx.offset == ho && idx.entered == he && idx.filter == bf && bf == gf);

  // the scan against the host restatement, and every planted slot among the hits
  const ricepp_amd::segment_hits hits = ricepp_amd::segment_scan(extent, idx.filter, cfg);
  std::vector<rpp_segment_hit> want(rpp_segment_positions(&c, eframes));
  uint64_t count = 0;
  CHECK(rpp_segment_host_scan(&c, extent.data(), eframes, bf.data(), want.data(), want.size(), &count) == RPP_OK);
  CHECK(hits.pos.size() == count && hits.hash.size() == count);
  for (uint64_t i = 0; i < count && i < hits.pos.size() && !failures; ++i)
    CHECK(hits.pos[i] == want[i].pos && hits.hash[i] == want[i].hash);
  size_t planted = 0;
  for (int a = 7; a < argc; ++a) {
    unsigned long long pos, off, frames;
    CHECK(std::sscanf(argv[a], "%llu:%llu:%llu", &pos, &off, &frames) == 3);
    for (uint64_t s = 0; s < slots && !failures; ++s)
      if (idx.entered[s] && idx.offset[s] >= off && idx.offset[s] + W <= off + frames) {
        const uint32_t p = static_cast<uint32_t>(pos + idx.offset[s] - off);
        bool found = false;
        for (uint32_t q : hits.pos) found = found || q == p;
        CHECK(found);
        // verify and extend on the host from this hit: the whole piece (or more) comes back
        const rpp_segment_candidate cand{0, 0, p, idx.offset[s], 0, static_cast<uint32_t>(eframes),
                                         static_cast<uint32_t>(bframes), 0};
        rpp_segment_match m{};
        CHECK(rpp_segment_host_extend(&c, extent.data(), block.data(), &cand, 1, &m) == RPP_OK);
        CHECK(m.size >= frames && m.pos <= pos && m.off <= off);
        ++planted;
      }
  }
  CHECK(argc == 7 || planted > 0);

  // an empty filter has no hit; an extent shorter than the window no position
  CHECK(ricepp_amd::segment_scan(extent, std::vector<uint64_t>(words, 0), cfg).pos.empty());
  CHECK(ricepp_amd::segment_scan(std::span<uint8_t const>(extent.data(), (W - 1) * g), idx.filter, cfg).pos.empty());
  CHECK(ricepp_amd::segment_index(std::span<uint8_t const>(block.data(), (W - 1) * g), cfg).hash.empty());
  bool thrown = false;
  try {
    ricepp_amd::segment_config bad = cfg;
    bad.filter_bits = 96;
    (void)ricepp_amd::segment_index(block, bad);
  } catch (std::runtime_error const& e) {
    thrown = std::strstr(e.what(), "Unsupported configuration") != nullptr;
  }
  CHECK(thrown);

  ricepp_amd::shutdown_facade();
  if (failures) {
    std::fprintf(stderr, "segment_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("segment_test: OK\n");
  return 0;
}
