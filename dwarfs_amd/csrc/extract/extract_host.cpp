// extract_host.cpp -- the definition of the file extraction and its sequential
// restatement.  The kernels of extract_kernels.hip give the same bytes and the
// same statuses.  Plain C++: the sanitizer test (tests/cpp/extract_test.cpp)
// compiles this file alone.
//
// Definition.  A file is a list of chunks (thrift/metadata.thrift, `chunk`:
// block, offset, size); the bulk readers walk every file's list and read the
// chunk bytes out of the decoded blocks (filesystem_extractor.cpp, dwarfsck's
// do_checksum).  Here the decoded blocks lie in one buffer (block b at
// block_offsets[b], block_sizes[b] bytes), the files in CSR form (file f holds
// the chunks file_first_chunk[f] .. file_first_chunk[f + 1]), and chunk c is
// written to out[chunk_dst[c] .. + size): chunk_dst is the exclusive scan of
// the chunk sizes laid over the files' places in `out`, nchunks + 1 entries.
//   hole       block == RPP_CHUNK_HOLE: `size` zero bytes, no source; block and
//              offset rules do not apply to it.
//   bad chunk  (extract_common.h, chunk_plan) any of
//                block >= nblocks and it is no hole;
//                offset + size > block_sizes[block], in 64 bits, or the block
//                itself runs past blocks_bytes;
//                chunk_dst[c] + size > out_bytes, or > chunk_dst[c + 1] (it
//                would run into its neighbour: chunk_dst must not decrease).
//              A bad chunk's destination bytes are left as they are, its file's
//              status becomes RPP_BAD_CHUNK, and every other chunk -- of the
//              same file and of every other file -- is copied as usual.
//   status     file_status[f] is RPP_OK or RPP_BAD_CHUNK; every entry is written.
//   size 0     a chunk of 0 bytes copies nothing but is still judged.
// Bytes of `out` that no chunk covers are not written.  This call refuses
// (RPP_INVALID_ARGUMENT) a file table that decreases, does not start at 0 or
// does not end at nchunks, and a null pointer where an array has entries; the
// kernels clamp a chunk's file into range instead.
#include <string.h>

#include "extract_common.h"

extern "C" uint64_t rpp_extract_tile_bytes(void) { return rpp_extract::kTileBytes; }

extern "C" uint64_t rpp_extract_workspace_bytes(uint64_t nchunks, uint32_t /*nfiles*/, uint64_t /*out_bytes*/) {
  const uint64_t n = rpp_extract::workspace_flags_at(nchunks) + rpp_extract::align16(nchunks);
  return n ? n : 16;
}

extern "C" int rpp_extract_host_gather(const uint8_t* blocks, uint64_t blocks_bytes, const uint64_t* block_offsets,
                                       const uint64_t* block_sizes, uint32_t nblocks, const rpp_chunk* chunks,
                                       const uint64_t* chunk_dst, uint64_t nchunks, const uint64_t* file_first_chunk,
                                       uint32_t nfiles, uint8_t* out, uint64_t out_bytes, int32_t* file_status) {
  using namespace rpp_extract;
  if (nfiles && (!file_first_chunk || !file_status)) return RPP_INVALID_ARGUMENT;
  if (nchunks && (!nfiles || !chunks || !chunk_dst)) return RPP_INVALID_ARGUMENT;
  if (nblocks && (!block_offsets || !block_sizes)) return RPP_INVALID_ARGUMENT;
  if ((blocks_bytes && !blocks) || (out_bytes && !out)) return RPP_INVALID_ARGUMENT;
  if (nfiles && (file_first_chunk[0] != 0 || file_first_chunk[nfiles] != nchunks)) return RPP_INVALID_ARGUMENT;
  for (uint32_t f = 0; f < nfiles; ++f)
    if (file_first_chunk[f] > file_first_chunk[f + 1]) return RPP_INVALID_ARGUMENT;
  for (uint32_t f = 0; f < nfiles; ++f) {
    file_status[f] = RPP_OK;
    for (uint64_t c = file_first_chunk[f]; c < file_first_chunk[f + 1]; ++c) {
      uint64_t src;
      const uint8_t plan = chunk_plan(chunks[c], chunk_dst[c], chunk_dst[c + 1], out_bytes, block_offsets, block_sizes,
                                      nblocks, blocks_bytes, &src);
      if (plan == kSkip) {
        file_status[f] = RPP_BAD_CHUNK;
      } else if (chunks[c].size) {
        if (plan == kZero) {
          memset(out + chunk_dst[c], 0, chunks[c].size);
        } else {
          memcpy(out + chunk_dst[c], blocks + src, chunks[c].size);
        }
      }
    }
  }
  return RPP_OK;
}
