// C++ test of the file extraction's host gather
// (dwarfs_amd/csrc/extract/extract_host.cpp), built by build_extract.sh with
// AddressSanitizer and UBSan into a program of its own: no GPU, no library,
// nothing loaded into another process.  It generates its families: every source
// phase x destination phase x size, chunks around the tile edges, block edges,
// holes, empty files and an empty batch, and bad chunks in the middle of good
// files.  Every array the call reads or writes is a heap block of exactly its
// size, so a byte read or written outside them stops the program.  Checked:
// every output byte and every status against a byte-by-byte restatement of the
// rules; the output is pre-filled, so bytes that must stay are seen to stay.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ricepp_amd.h"

static int failures = 0;
static const char* family = "";
#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (family %s)\n", __FILE__, __LINE__, #cond, family); \
      ++failures;                                                                                     \
    }                                                                                                 \
  } while (0)

template <typename T>
struct Exact {  // a heap block of exactly n elements (n == 0: one byte that is never offered)
  T* p;
  size_t n;
  explicit Exact(const std::vector<T>& v) : p(static_cast<T*>(std::malloc(v.empty() ? 1 : v.size() * sizeof(T)))), n(v.size()) {
    if (n) std::memcpy(p, v.data(), n * sizeof(T));
  }
  ~Exact() { std::free(p); }
  T* get() const { return n ? p : nullptr; }
};

static uint32_t rng_state = 2463534242u;
static uint8_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return uint8_t(rng_state >> 24);
}

struct Batch {
  std::vector<uint8_t> blocks;
  std::vector<uint64_t> block_offsets, block_sizes;
  std::vector<rpp_chunk> chunks;
  std::vector<uint64_t> chunk_dst, first{0};  // chunk_dst: every chunk's start; run() adds the last chunk's end
  uint64_t at = 0;        // where the next chunk goes
  uint64_t last_end = 0;  // where the last chunk's place ended

  void block(uint64_t n) {
    block_offsets.push_back(blocks.size());
    block_sizes.push_back(n);
    for (uint64_t i = 0; i < n; ++i) blocks.push_back(rnd());
  }
  // `room`: the bytes the chunk's place has (its size, unless the row claims more than its place)
  void chunk(uint32_t b, uint32_t off, uint64_t size, uint64_t room) {
    chunks.push_back(rpp_chunk{b, off, size});
    chunk_dst.push_back(at);
    at += room;
    last_end = at;
  }
  void chunk(uint32_t b, uint32_t off, uint64_t size) { chunk(b, off, size, size); }
  void hole(uint64_t size) { chunk(RPP_CHUNK_HOLE, 0, size); }
  void end_file(uint64_t gap) {  // the next file starts at least `gap` bytes on, on a 16-byte boundary
    first.push_back(chunks.size());
    at = (at + gap + 15) / 16 * 16;
  }
};

static void run(Batch& b, uint64_t tail) {
  const uint64_t out_bytes = b.at + tail;
  b.chunk_dst.push_back(b.last_end);
  std::vector<uint8_t> filled(out_bytes, 0xA5);
  std::vector<uint8_t> want(filled);
  std::vector<int32_t> want_status(b.first.size() - 1, RPP_OK);
  for (size_t f = 0; f + 1 < b.first.size(); ++f)
    for (uint64_t c = b.first[f]; c < b.first[f + 1]; ++c) {
      const rpp_chunk& ch = b.chunks[c];
      const uint64_t dst = b.chunk_dst[c], next = b.chunk_dst[c + 1];
      bool good = dst <= out_bytes && ch.size <= out_bytes - dst && next >= dst && ch.size <= next - dst;
      if (good && ch.block != RPP_CHUNK_HOLE)
        good = ch.block < b.block_sizes.size() && ch.offset <= b.block_sizes[ch.block] &&
               ch.size <= b.block_sizes[ch.block] - ch.offset;
      if (!good) {
        want_status[f] = RPP_BAD_CHUNK;
        continue;
      }
      for (uint64_t i = 0; i < ch.size; ++i)
        want[dst + i] = ch.block == RPP_CHUNK_HOLE ? 0 : b.blocks[b.block_offsets[ch.block] + ch.offset + i];
    }
  Exact<uint8_t> blocks(b.blocks), out(filled);
  Exact<uint64_t> boff(b.block_offsets), bsz(b.block_sizes), dst(b.chunk_dst), first(b.first);
  Exact<rpp_chunk> chunks(b.chunks);
  Exact<int32_t> status(std::vector<int32_t>(b.first.size() - 1, 77));
  const int st = rpp_extract_host_gather(blocks.get(), b.blocks.size(), boff.get(), bsz.get(), uint32_t(b.block_sizes.size()),
                                         chunks.get(), dst.get(), b.chunks.size(), first.get(), uint32_t(b.first.size() - 1),
                                         out.get(), out_bytes, status.get());
  CHECK(st == RPP_OK);
  CHECK(out_bytes == 0 || std::memcmp(out.p, want.data(), out_bytes) == 0);
  for (size_t f = 0; f < want_status.size(); ++f) CHECK(status.p[f] == want_status[f]);
}

int main() {
  const uint64_t tile = rpp_extract_tile_bytes();
  const uint64_t sizes[] = {0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 48};

  family = "align";
  {
    Batch b;
    b.block(1021);
    b.block(777);
    uint32_t k = 0;
    for (uint32_t sp = 0; sp < 16; ++sp)
      for (uint32_t dp = 0; dp < 16; ++dp)
        for (uint64_t size : sizes) {
          const uint32_t blk = k % 2;
          const uint32_t start = uint32_t((sp + 16 - b.block_offsets[blk] % 16) % 16 + 16 * (k % 37));
          b.chunk(1 - blk, 5 * (k % 100), dp);
          b.chunk(blk, start, size);
          b.end_file(0);
          ++k;
        }
    run(b, 0);
  }

  family = "tile_edges";
  for (uint64_t lead : {uint64_t(0), uint64_t(64)}) {
    Batch b;
    b.block(3 * tile + 101);
    b.block(2 * tile + 37);
    b.at = lead;
    b.chunk(0, 3, tile - 1 - lead);
    b.chunk(1, 7, 1);
    b.chunk(0, 11, 1);
    b.chunk(1, 1, tile - 2);
    b.chunk(0, 5, 2);
    b.chunk(0, 9, 2 * tile + 5);
    b.end_file(64);
    for (uint32_t k = 0; k < 200; ++k) b.chunk(k % 2, 13 + 3 * k, 1);
    b.end_file(64);
    for (uint32_t k = 0; k < 700; ++k) b.chunk(k % 2, 17 + 5 * k, 1 + k % 3);
    b.end_file(0);
    b.chunk(0, 0, tile);
    b.end_file(0);
    b.chunk(1, 0, tile + 1);
    b.end_file(64);
    run(b, 64);
  }

  family = "block_edges";
  {
    Batch b;
    b.block(333);
    b.block(4099);
    b.block(61);
    b.chunk(0, 0, 333);
    b.end_file(0);
    b.chunk(0, 0, 1);
    b.end_file(0);
    b.chunk(2, 0, 61);
    b.end_file(0);
    b.chunk(2, 60, 1);
    b.end_file(0);
    b.chunk(2, 29, 32);
    b.end_file(0);
    for (uint32_t f = 0; f < 24; ++f) {
      b.chunk(1, 40 * f, 100 + f);
      b.chunk(1, 7, 50);
      b.end_file(f % 3);
    }
    run(b, 0);
  }

  family = "holes";
  {
    Batch b;
    b.block(2 * tile + 9);
    b.block(999);
    b.hole(100);
    b.chunk(0, 5, 300);
    b.end_file(0);
    b.chunk(1, 0, 300);
    b.hole(77);
    b.end_file(0);
    b.chunk(0, 1, 50);
    b.hole(33);
    b.chunk(1, 2, 50);
    b.hole(1);
    b.chunk(0, 3, 5);
    b.end_file(0);
    b.hole(4097);
    b.end_file(0);
    b.chunk(0, 0, tile / 2 + 3);
    b.hole(tile + 100);
    b.chunk(1, 9, 20);
    b.end_file(0);
    b.chunk(1, 3, 10);
    b.hole(0);
    b.chunk(1, 13, 10);
    b.end_file(0);
    b.hole(0);
    b.end_file(0);
    run(b, 0);
  }

  family = "empty";
  {
    Batch b;
    b.block(500);
    b.block(123);
    b.chunk(0, 0, 40);
    b.end_file(0);
    b.end_file(0);  // a file with no chunks
    b.chunk(1, 3, 0);
    b.chunk(0, 500, 0);
    b.hole(0);
    b.chunk(1, 123, 0);
    b.end_file(0);
    b.end_file(0);
    b.chunk(1, 100, 23);
    b.end_file(0);
    b.end_file(0);
    run(b, 0);
    Batch none;  // an empty batch
    none.block(10);
    run(none, 0);
    Batch no_blocks;
    no_blocks.hole(5);
    no_blocks.end_file(0);
    no_blocks.end_file(0);
    run(no_blocks, 0);
  }

  family = "bad";
  for (int kind = 0; kind < 7; ++kind) {
    Batch b;
    b.block(700);
    b.block(300);
    auto good = [&](uint32_t k) {
      b.chunk(k % 2, 10 * k, 90 + k);
      b.hole(3);
      b.chunk(1 - k % 2, k, 35);
      b.end_file(0);
    };
    good(1);
    good(2);
    b.chunk(0, 0, 16);
    switch (kind) {
      case 0: b.chunk(2, 0, 50); break;                             // block == nblocks
      case 1: b.chunk(1, 251, 50); break;                           // one past the block
      case 2: b.chunk(0, 0xFFFFFFFFu, 2); break;                    // a 32-bit sum would wrap
      case 3: b.chunk(0, 701, 0); break;                            // size 0 behind the block
      case 4: b.chunk(1, 3, UINT64_C(1) << 40, 40); break;          // past the output
      case 5: b.chunk(RPP_CHUNK_HOLE, 0, ~UINT64_C(0), 24); break;  // a hole past the output
      case 6: b.chunk(1, 3, 41, 40); break;                         // into its neighbour
    }
    b.chunk(0, 16, 16);
    b.end_file(0);
    good(3);
    good(4);
    run(b, 0);
  }

  // argument rules
  family = "arguments";
  {
    uint64_t first_bad[3] = {0, 2, 1}, dst[3] = {0, 1, 2};
    rpp_chunk rows[2] = {{RPP_CHUNK_HOLE, 0, 1}, {RPP_CHUNK_HOLE, 0, 1}};
    uint8_t out[2];
    int32_t status[2];
    CHECK(rpp_extract_host_gather(nullptr, 0, nullptr, nullptr, 0, rows, dst, 2, first_bad, 2, out, 2, status) ==
          RPP_INVALID_ARGUMENT);
    CHECK(rpp_extract_host_gather(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr) ==
          RPP_OK);
    CHECK(rpp_extract_workspace_bytes(1000, 3, 5) % 16 == 0 && tile % 16 == 0);
  }

  if (failures) {
    std::fprintf(stderr, "extract_test: %d failures\n", failures);
    return 1;
  }
  std::printf("extract_test: OK\n");
  return 0;
}
