// incompressible_long_host.cpp -- rpp_incompressible_host_scan under the
// Zstandard encoder's `long` word: the scan of incompressible_host.cpp (defined
// at its top) with the sizes of rpp_zstd_host_encode_long.  A file of its own
// so that the host scan links without the long-distance matcher.  Plain C++.
#include "../lz4_common.h"
#include "../zstd_enc_common.h"
#include "../zstd_long_common.h"
#include "incompressible_host_impl.h"
#include "ricepp_amd.h"

extern "C" int rpp_incompressible_host_scan_long(const uint8_t* in, const uint64_t* in_offsets,
                                                 const uint64_t* in_bytes, uint32_t npieces,
                                                 const uint32_t* piece_base, uint32_t nextents, double max_ratio,
                                                 uint32_t generate_fragments, uint32_t options, uint32_t search,
                                                 uint32_t long_mode, uint64_t* sizes, uint32_t* verdicts,
                                                 uint64_t* totals, uint64_t* frag_rows, uint32_t* frag_count,
                                                 int32_t* status) {
  if ((options & ~rpp_zstd::kEncOptionsMask) || !rpp_lz4::search_valid(search) || long_mode > 1)
    return RPP_INVALID_ARGUMENT;
  return rpp_incompressible::host_scan(
      in, in_offsets, in_bytes, npieces, piece_base, nextents, max_ratio, generate_fragments,
      long_mode ? rpp_zstd_long::kLongMaxBlock : rpp_lz4::kMaxBlock,
      [=](const uint8_t* piece, uint64_t n, uint8_t* frame, uint64_t capacity, uint64_t* size) {
        return rpp_zstd_host_encode_long(piece, n, options, search, long_mode, frame, capacity, size, nullptr);
      },
      sizes, verdicts, totals, frag_rows, frag_count, status);
}
