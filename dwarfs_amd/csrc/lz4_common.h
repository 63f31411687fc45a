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

// extension bytes behind a token nibble that stands for `v` (a literal length, or a match length - 4)
RPP_LZ4_HD inline uint32_t ext_bytes(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }

// bytes of one sequence with `lit` literals and a match of `len` bytes
RPP_LZ4_HD inline uint32_t seq_bytes(uint32_t lit, uint32_t len) {
  return 1 + ext_bytes(lit) + lit + 2 + ext_bytes(len - kMinMatch);
}

}  // namespace rpp_lz4
