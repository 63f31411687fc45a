// extract_kernels.hip -- file extraction on the GPU (gfx950): chunks of decoded
// blocks become files.  The definition is at the top of extract_host.cpp, the
// sequential restatement that gives the same bytes and statuses; the chunk
// rules themselves are one function shared with it (extract_common.h).
//
// Two launches behind a memset of the file statuses:
//   validate  one lane per chunk: the rules (chunk_plan), the chunk's first
//             source byte and its copy flag (skip / copy / zero) into the
//             workspace; a bad chunk finds its file by binary search in the CSR
//             table and marks it with an atomic max on the status word read as
//             unsigned, under which any error outranks RPP_OK.
//   gather    tiled over the DESTINATION: one workgroup of 256 lanes owns one
//             tile of 16 KiB of output (rpp_extract::kTileBytes), whatever the
//             chunks look like, so one 1 GiB chunk and a million 64-byte chunks
//             both spread over the whole device.  It finds the last chunk that
//             starts at or before its tile by binary search in d_chunk_dst and
//             walks the chunks from there in batches of 255 staged in LDS
//             (destination, end, source, flag; a skipped chunk's range is
//             empty), until a batch's successor starts at or behind the tile's
//             end.  A lane owns the 16-byte granules lane, lane + 256, ... of
//             the tile (the output is 16-aligned, so granules are too, and no
//             byte has two writers).  It looks its granule's chunk up in the
//             staged batch (binary search in LDS: one step for a tile inside
//             one large chunk, eight for 255 small ones).  A granule that lies
//             inside one chunk is one 16-byte store: zeros for a hole, else two
//             aligned 16-byte loads around the source position, funnel-shifted
//             into place (dword select + v_alignbit; the second load is left
//             out when the source is 16-aligned).  Any other granule -- a
//             chunk's head or tail, several small chunks, a gap between files --
//             is written byte by byte, each byte taken from the aligned dword
//             that holds it, and bytes outside every good chunk are not stored.
// Loads stay inside [0, round_up(blocks_bytes, 16)): an aligned 16-byte load
// that holds a byte below blocks_bytes ends at or below that bound.  Stores are
// guarded by the staged chunk's own validated range, so a table that breaks the
// ordering rule can misplace nothing outside a good chunk's destination.
// No inline assembly; 64-bit variable shifts are avoided.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "extract_common.h"

namespace {

using namespace rpp_extract;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kGranule = 16;
constexpr uint32_t kGranulesPerLane = uint32_t(kTileBytes / kGranule / kThreads);
constexpr uint32_t kBatch = kThreads - 1;  // chunks per staged batch; the last lane stages the successor's start
static_assert(kGranulesPerLane * kGranule * kThreads == kTileBytes, "a tile is a whole number of granule rounds");

__global__ __launch_bounds__(kThreads) void rpp_extract_validate_kernel(
    const rpp_chunk* __restrict__ chunks, const uint64_t* __restrict__ chunk_dst, uint64_t nchunks,
    const uint64_t* __restrict__ file_first, uint32_t nfiles, const uint64_t* __restrict__ block_offsets,
    const uint64_t* __restrict__ block_sizes, uint32_t nblocks, uint64_t blocks_bytes, uint64_t out_bytes,
    uint64_t* __restrict__ ws_src, uint8_t* __restrict__ ws_flag, int32_t* file_status) {
  const uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= nchunks) return;
  uint64_t src;
  const uint8_t plan = chunk_plan(chunks[c], chunk_dst[c], chunk_dst[c + 1], out_bytes, block_offsets, block_sizes,
                                  nblocks, blocks_bytes, &src);
  ws_src[c] = src;
  ws_flag[c] = plan;
  if (plan != kSkip) return;
  // the chunk's file: the first f whose successor starts behind c (the last file when the table is broken)
  uint32_t lo = 0, hi = nfiles - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (file_first[mid + 1] > c) hi = mid; else lo = mid + 1;
  }
  atomicMax(reinterpret_cast<unsigned int*>(file_status) + lo, static_cast<unsigned int>(RPP_BAD_CHUNK));
}

// the byte at q, from the aligned dword that holds it
__device__ inline uint8_t load_byte(const uint8_t* __restrict__ blocks, uint64_t q) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(blocks + (q & ~uint64_t(3)));
  return uint8_t(w >> ((uint32_t(q) & 3u) * 8u));
}

// the 16 bytes at s (any alignment), from the aligned 16-byte words around it
__device__ inline uint4 load_granule(const uint8_t* __restrict__ blocks, uint64_t s) {
  const uint32_t sh = uint32_t(s) & 15u;
  const uint4* p = reinterpret_cast<const uint4*>(blocks + (s - sh));
  const uint4 a = p[0];
  if (sh == 0) return a;
  const uint4 b = p[1];  // (holds the byte s + 15, which lies in the chunk's block)
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const uint32_t bits = (sh & 3u) * 8u, d = sh >> 2;
  uint32_t v[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = __funnelshift_r(w[k], w[k + 1], bits);
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = d == 0 ? v[k] : d == 1 ? v[k + 1] : d == 2 ? v[k + 2] : v[k + 3];
  return make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(kThreads) void rpp_extract_gather_kernel(
    const uint8_t* __restrict__ blocks, const rpp_chunk* __restrict__ chunks, const uint64_t* __restrict__ chunk_dst,
    uint64_t nchunks, const uint64_t* __restrict__ ws_src, const uint8_t* __restrict__ ws_flag,
    uint8_t* __restrict__ out, uint64_t out_bytes) {
  __shared__ uint64_t s_dst[kThreads];  // [n] is the successor's start
  __shared__ uint64_t s_end[kBatch];
  __shared__ uint64_t s_src[kBatch];
  __shared__ uint8_t s_flag[kBatch];
  const uint32_t t = threadIdx.x;
  const uint64_t tile_lo = uint64_t(blockIdx.x) * kTileBytes;
  const uint64_t tile_hi = tile_lo + kTileBytes < out_bytes ? tile_lo + kTileBytes : out_bytes;

  // the last chunk that starts at or before the tile (chunk 0 when none does)
  uint64_t lo = 0, hi = nchunks;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (chunk_dst[mid] <= tile_lo) lo = mid + 1; else hi = mid;
  }
  uint64_t cb = lo ? lo - 1 : 0;

  for (;;) {
    const uint32_t n = nchunks - cb < kBatch ? uint32_t(nchunks - cb) : kBatch;
    if (t <= n) {
      const uint64_t d = chunk_dst[cb + t];
      s_dst[t] = d;
      if (t < n) {
        const uint8_t flag = ws_flag[cb + t];
        s_flag[t] = flag;
        s_src[t] = ws_src[cb + t];
        s_end[t] = flag == kSkip ? d : d + chunks[cb + t].size;  // (validated: no wrap, at most out_bytes)
      }
    }
    __syncthreads();
    const uint64_t batch_lo = s_dst[0], batch_hi = s_dst[n];  // this batch answers for [batch_lo, batch_hi)
#pragma unroll
    for (uint32_t k = 0; k < kGranulesPerLane; ++k) {
      const uint64_t g = tile_lo + uint64_t(t + k * kThreads) * kGranule;
      uint64_t r_lo = g > batch_lo ? g : batch_lo;
      uint64_t r_hi = g + kGranule < batch_hi ? g + kGranule : batch_hi;
      if (r_hi > tile_hi) r_hi = tile_hi;
      if (r_lo >= r_hi) continue;
      uint32_t j = 0, jh = n;  // the last staged chunk that starts at or before r_lo
      while (jh - j > 1) {
        const uint32_t mid = (j + jh) / 2;
        if (s_dst[mid] <= r_lo) j = mid; else jh = mid;
      }
      if (s_dst[j] <= g && g + kGranule <= s_end[j]) {  // the whole granule inside one good chunk
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (s_flag[j] == kCopy) v = load_granule(blocks, s_src[j] + (g - s_dst[j]));
        *reinterpret_cast<uint4*>(out + g) = v;
        continue;
      }
      for (uint64_t p = r_lo; p < r_hi; ++p) {
        while (j + 1 < n && s_dst[j + 1] <= p) ++j;
        if (p >= s_dst[j] && p < s_end[j])
          out[p] = s_flag[j] == kCopy ? load_byte(blocks, s_src[j] + (p - s_dst[j])) : uint8_t(0);
      }
    }
    __syncthreads();
    cb += n;
    if (cb >= nchunks || batch_hi >= tile_hi) break;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int rpp_extract_gather_batch(const uint8_t* d_blocks, uint64_t blocks_bytes, const uint64_t* d_block_offsets,
                                        const uint64_t* d_block_sizes, uint32_t nblocks, const rpp_chunk* d_chunks,
                                        const uint64_t* d_chunk_dst, uint64_t nchunks,
                                        const uint64_t* d_file_first_chunk, uint32_t nfiles, uint8_t* d_out,
                                        uint64_t out_bytes, int32_t* d_file_status, void* d_workspace,
                                        uint64_t workspace_bytes, void* stream) {
  if (nfiles && (!d_file_first_chunk || !d_file_status)) return RPP_INVALID_ARGUMENT;
  if (nchunks && (!nfiles || !d_chunks || !d_chunk_dst || !d_workspace)) return RPP_INVALID_ARGUMENT;
  if (nblocks && (!d_block_offsets || !d_block_sizes)) return RPP_INVALID_ARGUMENT;
  if ((blocks_bytes && !d_blocks) || (out_bytes && !d_out)) return RPP_INVALID_ARGUMENT;
  if (!aligned16(d_blocks) || !aligned16(d_out) || !aligned16(d_workspace)) return RPP_INVALID_ARGUMENT;
  if (nchunks && workspace_bytes < rpp_extract_workspace_bytes(nchunks, nfiles, out_bytes)) return RPP_INVALID_ARGUMENT;
  const uint64_t vblocks = (nchunks + kThreads - 1) / kThreads, tiles = (out_bytes + kTileBytes - 1) / kTileBytes;
  if (vblocks > 0x7fffffffu || tiles > 0x7fffffffu) return RPP_INVALID_ARGUMENT;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nfiles && hipMemsetAsync(d_file_status, 0, sizeof(int32_t) * uint64_t(nfiles), s) != hipSuccess)
    return RPP_HIP_ERROR;
  if (nchunks == 0) return RPP_OK;
  uint64_t* ws_src = static_cast<uint64_t*>(d_workspace);
  uint8_t* ws_flag = static_cast<uint8_t*>(d_workspace) + workspace_flags_at(nchunks);
  hipLaunchKernelGGL(rpp_extract_validate_kernel, dim3(uint32_t(vblocks)), dim3(kThreads), 0, s, d_chunks, d_chunk_dst,
                     nchunks, d_file_first_chunk, nfiles, d_block_offsets, d_block_sizes, nblocks, blocks_bytes,
                     out_bytes, ws_src, ws_flag, d_file_status);
  if (tiles)
    hipLaunchKernelGGL(rpp_extract_gather_kernel, dim3(uint32_t(tiles)), dim3(kThreads), 0, s, d_blocks, d_chunks,
                       d_chunk_dst, nchunks, ws_src, ws_flag, d_out, out_bytes);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}
