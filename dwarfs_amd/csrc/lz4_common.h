// lz4_common.h -- the constants and the small functions that the LZ4 kernels
// (lz4_kernels.hip) and their sequential restatement (lz4_host.cpp) share, so
// that the two cannot drift apart (not part of the C ABI; plain C++, no HIP).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RPP_LZ4_HD __host__ __device__
#else
#define RPP_LZ4_HD
#endif

namespace rpp_lz4 {

constexpr uint32_t kChunk = 32768;       // bytes of a block that one wave searches
constexpr uint32_t kStep = 64;           // positions looked up, then inserted, together
constexpr uint32_t kHashBits = 12;       // the chunk's LDS table: 4096 entries
constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMaxOffset = 65535;
constexpr uint32_t kLastLiterals = 5;    // the block's last 5 bytes are literals
constexpr uint32_t kMatchStartGap = 12;  // the last match starts at least 12 bytes before the end
constexpr uint64_t kMaxBlock = UINT64_C(1) << 30;
constexpr uint32_t kSeqsPerChunk = kChunk / kMinMatch;

RPP_LZ4_HD inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// The search word (defined at the top of lz4_host.cpp): 0 is the one-candidate greedy search; else
// depth | kSearchLazy with a depth of 1, 2, 4 or 8 candidates per hash value.
constexpr uint32_t kSearchLazy = 0x100;
constexpr uint32_t kMaxDepth = 8;
// A candidate's score is its common prefix up to this many bytes: one cache line, and one turn of the whole-wave
// compare that extends the match taken.  Two candidates that both agree this far are told apart by position
// alone, and a match this long is never given up for the next position's: a byte more would gain under 2 %.
constexpr uint32_t kDeepCap = 64;

RPP_LZ4_HD inline bool search_valid(uint32_t search) {
  const uint32_t d = search & ~kSearchLazy;
  return search == 0 || d == 1 || d == 2 || d == 4 || d == 8;
}

// extension bytes behind a token nibble that stands for `v` (a literal length, or a match length - 4)
RPP_LZ4_HD inline uint32_t ext_bytes(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }

// bytes of one sequence with `lit` literals and a match of `len` bytes
RPP_LZ4_HD inline uint32_t seq_bytes(uint32_t lit, uint32_t len) {
  return 1 + ext_bytes(lit) + lit + 2 + ext_bytes(len - kMinMatch);
}

}  // namespace rpp_lz4
