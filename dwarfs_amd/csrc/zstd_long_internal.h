// zstd_long_internal.h -- the long-distance matcher of the Zstandard encoder
// as other translation units may use it (not part of the C ABI).  The matcher
// is defined at the top of zstd_long_host.cpp; the host form lives there, the
// kernels in zstd_long.hip.
#pragma once

#include <stdint.h>

#include <vector>

#include "lz4_internal.h"

namespace rpp_zstd {

// The frame of a block of n bytes from its sequences (zstd_encode_host.cpp): what rpp_zstd_host_encode_search
// writes behind its search.  `out` holds rpp_zstd_bound(n) bytes.
void write_frame(const uint8_t* in, uint32_t n, uint32_t options, const std::vector<rpp_lz4::Seq>& seqs, uint8_t* out,
                 uint64_t* out_bytes, uint32_t* bad_ratio);

}  // namespace rpp_zstd

namespace rpp_zstd_long {

// the long matches of a block of n <= kLongMaxBlock bytes, in order (host memory)
void find_long(const uint8_t* in, uint32_t n, std::vector<rpp_lz4::Seq>& longs);
// the final list of a block from the short search's sequences and its long matches
void merge(const std::vector<rpp_lz4::Seq>& shorts, const std::vector<rpp_lz4::Seq>& longs,
           std::vector<rpp_lz4::Seq>& out);
// the sequences of a block under (search, long_mode): what the frame is written from
void sequences(const uint8_t* in, uint32_t n, uint32_t search, uint32_t long_mode, std::vector<rpp_lz4::Seq>& out);

// the kernels' side: for translation units that have included <hip/hip_runtime.h> and say so
#if defined(RPP_LZ4_KERNEL_SIDE)
struct LongWs {
  uint64_t* n_eff;      // [nblocks] the block's size, or one that the prep kernel refuses (over kLongMaxBlock)
  uint64_t* tab_base;   // [nblocks + 1] first table entry of block b
  uint32_t* tab;        // [long_table_entries] the tables
  uint32_t* lcnt;       // per chunk: long matches
  uint2* lseqs;         //   [kLongPerChunk] their records
  uint32_t* mcnt;       // per chunk: sequences of the final list
  uint2* mseqs;         //   [kSeqsPerChunk] the final list
  uint64_t tab_entries;
};

uint64_t workspace_bytes(uint64_t total_bytes, uint32_t nblocks);
LongWs carve(void* p, uint64_t total_bytes, uint32_t nblocks);
// In front of the prep kernel on `stream`: n_eff, the table bases, the tables cleared.  The launches behind it
// take ws.n_eff in d_in_bytes' place.
void launch_prepare(const uint64_t* d_in_bytes, uint32_t nblocks, const LongWs& lws, void* stream);
// Behind the short search on `stream`: index, find and merge.  The chunk's final list is lws.mcnt, lws.mseqs.
void launch_match(const uint8_t* d_in, const uint64_t* d_in_offsets, uint32_t nblocks, const rpp_lz4::EncodeWs& ws,
                  const LongWs& lws, void* stream);
#endif

}  // namespace rpp_zstd_long
