// zstd_long_common.h -- the constants and the small functions that the
// long-distance kernels of the Zstandard encoder (zstd_long.hip) and their
// sequential restatement (zstd_long_host.cpp) share, so that the two cannot
// drift apart.  The definition they add up to is stated at the top of
// zstd_long_host.cpp.  Plain C++, no HIP.
#ifndef RPP_ZSTD_LONG_COMMON_H
#define RPP_ZSTD_LONG_COMMON_H

#include "lz4_common.h"
#include "zstd_common.h"

namespace rpp_zstd_long {

constexpr uint32_t kLongWindow = 32;    // bytes hashed
constexpr uint32_t kLongGrid = 32;      // spacing of the indexed positions
constexpr uint32_t kLongMinMatch = 64;  // a long match is at least this long
// The largest block with long = 1.  The largest offset value is then 2^27 + 2: its code is 27, which the Predefined
// offset table states (up to 28) and which fits the 6 bits a code has in the entropy kernel's record; and 2^27 is
// the largest window that a stock streaming decoder accepts without being asked.
constexpr uint64_t kLongMaxBlock = UINT64_C(1) << 27;
constexpr uint32_t kLongEmpty = 0xffffffffu;                                  // a table entry that holds no position
constexpr uint32_t kLongPerChunk = rpp_lz4::kChunk / kLongMinMatch;          // long matches of a chunk, at most
constexpr uint32_t kLongTableLogMin = 6;
static_assert(kLongWindow % 4 == 0 && kLongWindow == 32, "long_hash takes eight words");
static_assert(kLongMinMatch >= kLongWindow + kLongGrid - 1, "a copy of kLongMinMatch bytes holds a whole grid window");

// The accuracy of a block's table: the smallest log >= kLongTableLogMin with 2^log >= n / 16, which is two entries
// per grid position, rounded up to a power of two.  At most 23 for n <= kLongMaxBlock.
RPP_ZSTD_HD uint32_t long_table_log(uint64_t n) {  // n <= kLongMaxBlock
  const uint32_t want = uint32_t(n >> 4);
  uint32_t log = kLongTableLogMin;
  while ((1u << log) < want) ++log;
  return log;
}

// Entries that the tables of nblocks blocks of total_bytes bytes together take, at most (2^log < max(128, n / 8)).
RPP_ZSTD_HD uint64_t long_table_entries(uint64_t total_bytes, uint32_t nblocks) {
  return total_bytes / 8 + (UINT64_C(2) << kLongTableLogMin) * nblocks;
}

// the hash of a window of kLongWindow bytes, given as its eight little-endian words
RPP_ZSTD_HD uint32_t long_hash(const uint32_t* w) {
  uint32_t h = 0;
  for (uint32_t k = 0; k < kLongWindow / 4; ++k) h = ((h << 5 | h >> 27) ^ w[k]) * 2654435761u;
  h ^= h >> 16;
  return h * 0x85EBCA6Bu;
}

RPP_ZSTD_HD uint32_t long_slot(uint32_t hash, uint32_t log) { return hash >> (32 - log); }

// The widened workspace record of a match: (pos - chunk start) | offset's low half << 16, length | offset's high
// half << 16.  A length is at most kChunk = 2^15, so it leaves the upper 16 bits free; the short search writes 0
// there, and its records read the same through these accessors.
RPP_ZSTD_HD uint32_t rec_x(uint32_t rel, uint32_t off) { return rel | (off & 0xffffu) << 16; }
RPP_ZSTD_HD uint32_t rec_y(uint32_t len, uint32_t off) { return len | (off >> 16) << 16; }
RPP_ZSTD_HD uint32_t rec_rel(uint32_t x) { return x & 0xffffu; }
RPP_ZSTD_HD uint32_t rec_len(uint32_t y) { return y & 0xffffu; }
RPP_ZSTD_HD uint32_t rec_off(uint32_t x, uint32_t y) { return x >> 16 | (y >> 16) << 16; }
static_assert(rpp_lz4::kChunk <= 0xffffu, "a length leaves the record's upper half free");

}  // namespace rpp_zstd_long

#endif  // RPP_ZSTD_LONG_COMMON_H
