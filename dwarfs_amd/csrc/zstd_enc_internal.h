// zstd_enc_internal.h -- the Zstandard encoder's first stages as other
// translation units may use them (not part of the C ABI): the incompressible
// categorizer needs the encoder's sizes and none of its bytes.  The launches
// live in zstd_encode.hip; the encoder is defined at the top of
// zstd_encode_host.cpp.  For translation units that have included
// <hip/hip_runtime.h> and lz4_internal.h with RPP_LZ4_KERNEL_SIDE.
#pragma once

#include <stdint.h>

#include "lz4_internal.h"

namespace rpp_zstd {

struct EntropyStage {
  rpp_lz4::EncodeWs ws;        // chunk_base, ok: which chunks are block b's
  const uint32_t* block_size;  // per chunk: Block_Size of its Zstandard block (Raw: the chunk's bytes)
};

// The launches of rpp_zstd_encode_batch_long before `place` on `stream`: prep, search, with long_mode the
// long-distance matcher (zstd_long.hip), and entropy, over the 16-aligned workspace of
// rpp_zstd_encode_workspace_bytes_long(total_bytes, nblocks, long_mode).  The arguments are valid by that call's
// rules (the caller has checked them).  The prep kernel writes d_status and zeroes d_out_bytes and d_flags; with
// long_mode a block above RPP_ZSTD_LONG_MAX_BLOCK has the status of an over-size block and no chunks.
EntropyStage launch_search_entropy(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                   uint32_t nblocks, uint32_t options, uint32_t search, uint32_t long_mode,
                                   uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                   void* d_workspace, void* stream);

}  // namespace rpp_zstd
