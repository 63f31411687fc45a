// lz4_internal.h -- the LZ4 encoder's match search as other translation units
// may use it (not part of the C ABI): the Zstandard encoder writes the same
// sequences in another format.  The search is defined at the top of
// lz4_host.cpp; the host form lives there, the kernels in lz4_kernels.hip.
#pragma once

#include <stdint.h>

#include <vector>

#include "lz4_common.h"

namespace rpp_lz4 {

struct Seq {  // a match of `len` bytes at `pos`, `off` bytes back
  uint32_t pos, len, off;
};

// the sequences of a block of n bytes, in order (host memory)
void find_sequences(const uint8_t* in, uint32_t n, std::vector<Seq>& seqs);
// ... under a search word (valid by search_valid; 0 is the call above)
void find_sequences(const uint8_t* in, uint32_t n, std::vector<Seq>& seqs, uint32_t search);

// the kernels' side: for translation units that have included <hip/hip_runtime.h> and say so
#if defined(RPP_LZ4_KERNEL_SIDE)
struct EncodeWs {
  uint32_t* chunk_base;  // [nblocks + 1] first chunk of block b
  uint32_t* ok;          // [1] the batch fits the workspace
  uint32_t* fin_anchor;  // [nblocks] where the block's last literal run starts
  uint32_t* fin_off;     // [nblocks] ... and its place in the block's output
  uint32_t* cnt;         // per chunk: sequences
  uint32_t* first_pos;   //   position of the first match
  uint32_t* last_end;    //   end of the last match
  uint32_t* body;        //   bytes of the sequences without the first one's literals
  uint32_t* carry;       //   end of the last match before the chunk
  uint32_t* out_off;     //   place of the chunk's first sequence in the block's output
  uint2* seqs;           // [chunks * kSeqsPerChunk] (pos - chunk start) | offset << 16, length
  uint32_t max_chunks;
};

inline uint64_t max_chunks_of(uint64_t total_bytes, uint32_t nblocks) { return total_bytes / kChunk + nblocks; }

// The search workspace laid out in the first rpp_lz4_encode_workspace_bytes(total_bytes, nblocks) bytes at
// d_workspace (16-aligned).
EncodeWs carve_workspace(void* d_workspace, uint64_t total_bytes, uint32_t nblocks);

// The prep and search launches of rpp_lz4_encode_batch on `stream`: statuses, zeroed sizes and flags, the chunk
// counts, and every chunk's sequence list.
void launch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes, uint32_t nblocks,
                   const EncodeWs& ws, uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, void* stream);
// ... under a search word (valid by search_valid): 0 is the call above, any other word runs
// rpp_lz4_deep_search_kernel (lz4_search_deep.hip) in the search kernel's place.
void launch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes, uint32_t nblocks,
                   const EncodeWs& ws, uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint32_t search,
                   void* stream);
// the deep search kernel alone, behind the prep kernel on `stream` (search != 0)
void launch_deep_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                        uint32_t nblocks, const EncodeWs& ws, uint32_t search, void* stream);

// the block of global chunk g: the last b with chunk_base[b] <= g
__device__ inline uint32_t block_of_chunk(const uint32_t* chunk_base, uint32_t nblocks, uint32_t g) {
  uint32_t lo = 0, hi = nblocks;  // chunk_base[lo] <= g < chunk_base[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (chunk_base[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}
#endif

}  // namespace rpp_lz4
