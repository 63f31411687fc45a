// extract_common.h -- the chunk rules of the file extraction, shared by the
// host definition (extract_host.cpp) and the validate kernel
// (extract_kernels.hip) so that the two cannot drift apart.  Plain C++.
#ifndef RPP_EXTRACT_COMMON_H
#define RPP_EXTRACT_COMMON_H

#include <stdint.h>

#include "ricepp_amd.h"

#if defined(__HIPCC__)
#define RPP_EXTRACT_HD __host__ __device__
#else
#define RPP_EXTRACT_HD
#endif

namespace rpp_extract {

// The gather kernel's tile: one workgroup writes this many consecutive bytes of the output.
constexpr uint64_t kTileBytes = 16384;

// The workspace: per chunk its first source byte in the blocks buffer (uint64), then per chunk the copy flag
// (one byte: kSkip, kCopy or kZero below), each array rounded up to 16 bytes.
RPP_EXTRACT_HD inline uint64_t align16(uint64_t n) { return (n + 15) & ~uint64_t(15); }
RPP_EXTRACT_HD inline uint64_t workspace_flags_at(uint64_t nchunks) { return align16(8 * nchunks); }

// what the gather does with a chunk (its copy flag)
constexpr uint8_t kSkip = 0;  // bad: its destination is left as it is
constexpr uint8_t kCopy = 1;
constexpr uint8_t kZero = 2;  // a hole

// The verdict for chunk `ch` whose destination is [dst, dst + ch.size) and whose successor starts at next_dst;
// *src gets the chunk's first byte in the blocks buffer (kCopy only).  Every comparison is written so that no
// sum can wrap.
RPP_EXTRACT_HD inline uint8_t chunk_plan(const rpp_chunk& ch, uint64_t dst, uint64_t next_dst, uint64_t out_bytes,
                                         const uint64_t* block_offsets, const uint64_t* block_sizes, uint32_t nblocks,
                                         uint64_t blocks_bytes, uint64_t* src) {
  *src = 0;
  if (dst > out_bytes || ch.size > out_bytes - dst) return kSkip;  // runs past the output
  if (next_dst < dst || ch.size > next_dst - dst) return kSkip;    // runs into its neighbour
  if (ch.block == RPP_CHUNK_HOLE) return kZero;
  if (ch.block >= nblocks) return kSkip;
  const uint64_t at = block_offsets[ch.block], n = block_sizes[ch.block];
  if (at > blocks_bytes || n > blocks_bytes - at) return kSkip;  // the block itself passes the buffer
  if (ch.offset > n || ch.size > n - ch.offset) return kSkip;    // offset + size > the block's size
  *src = at + ch.offset;
  return kCopy;
}

}  // namespace rpp_extract

#endif  // RPP_EXTRACT_COMMON_H
