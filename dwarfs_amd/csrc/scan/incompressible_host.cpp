// incompressible_host.cpp -- the incompressible categorizer's definition and
// its sequential restatement.  The kernels of incompressible_kernels.hip
// restate the rules below and give the same numbers.  Plain C++: the sanitizer
// test (tests/cpp/incompressible_test.cpp) compiles this file with
// zstd_encode_host.cpp and lz4_host.cpp.
//
// Definition (mkdwarfs's `incompressible` categorizer,
// src/writer/categorizer/incompressible_categorizer.cpp: data_extent_fragments::
// compress, add_fragment, get_fragments), for one *extent*, a contiguous run of
// file data, under {block_size, generate_fragments, max_ratio, options, search}:
//   pieces     the extent is cut into pieces of block_size bytes; the last one
//              may be shorter.  An extent of 0 bytes has no piece.  The caller
//              cuts: a call takes the pieces (offset and size in one buffer) and
//              per extent the range of its pieces, piece_base[e] ..
//              piece_base[e + 1].
//   size       a piece's compressed size is the size of the ONE frame that this
//              project's Zstandard encoder writes for it under the options and
//              the search word (rpp_zstd_host_encode_search's out_bytes, frame
//              header included, as ZSTD_compressCCtx's return value includes
//              its header in the reference).  It is not libzstd's size: the
//              reference's zstd level has no counterpart; (0, 0) is the fastest
//              path.  The kernels compute it without writing the frame: frame
//              header bytes + the sum over the piece's chunks of 3 + Block_Size.
//   verdict    a piece of n bytes is incompressible (1) iff
//              double(size) >= max_ratio * double(n), in IEEE double: one
//              multiplication and one comparison, the same on host and device.
//   totals     per extent five numbers: total_in (the sum of n), total_out (the
//              sum of the sizes), blocks (its pieces), incompressible_blocks,
//              and the single-fragment verdict: 1 iff blocks > 0 and
//              double(total_out) >= max_ratio * double(total_in).
//   fragments  with generate_fragments, the run-length list of (category, bytes)
//              over the extent's pieces in order: neighbouring pieces of one
//              verdict merge.  Category 0 is the default, 1 incompressible.  The
//              rows of extent e start at row piece_base[e] (a run list is never
//              longer than the piece list) and frag_count[e] says how many there
//              are; rows behind them are not written.  Without
//              generate_fragments frag_count[e] is 0 and no row is written.
// What becomes of an extent's numbers (the single fragment that stands in for
// an empty list, force_single_default, holes, min_input_size) is get_fragments,
// add_hole and result() of the reference, restated in dwarfs_amd/categorize.py.
// A piece larger than RPP_LZ4_MAX_BLOCK has the status RPP_INVALID_ARGUMENT, size 0
// and verdict 0; every other piece RPP_OK.  piece_base does not decrease and
// ends at or below npieces: this call refuses anything else, the kernels clamp.
#include <vector>

#include "../lz4_common.h"
#include "ricepp_amd.h"
#include "../zstd_enc_common.h"
#include "incompressible_host_impl.h"

static_assert(RPP_INCOMPRESSIBLE_TOTALS == 5, "total_in, total_out, blocks, incompressible_blocks, single verdict");

extern "C" int rpp_incompressible_host_scan(const uint8_t* in, const uint64_t* in_offsets, const uint64_t* in_bytes,
                                            uint32_t npieces, const uint32_t* piece_base, uint32_t nextents,
                                            double max_ratio, uint32_t generate_fragments, uint32_t options,
                                            uint32_t search, uint64_t* sizes, uint32_t* verdicts, uint64_t* totals,
                                            uint64_t* frag_rows, uint32_t* frag_count, int32_t* status) {
  if ((options & ~rpp_zstd::kEncOptionsMask) || !rpp_lz4::search_valid(search)) return RPP_INVALID_ARGUMENT;
  return rpp_incompressible::host_scan(
      in, in_offsets, in_bytes, npieces, piece_base, nextents, max_ratio, generate_fragments, rpp_lz4::kMaxBlock,
      [=](const uint8_t* piece, uint64_t n, uint8_t* frame, uint64_t capacity, uint64_t* size) {
        return rpp_zstd_host_encode_search(piece, n, options, search, frame, capacity, size, nullptr);
      },
      sizes, verdicts, totals, frag_rows, frag_count, status);
}
