// incompressible_kernels.hip -- the incompressible categorizer on the GPU
// (gfx950).  The definition is at the top of incompressible_host.cpp, the
// sequential restatement that gives the same numbers.
//
// One categorizer piece is one block of the Zstandard encoder.  Five launches:
// the encoder's prep, search and entropy (zstd_enc_internal.h: the kernels of
// rpp_zstd_encode_batch_search, unchanged, which leave every chunk's
// Block_Size in the workspace), then
//   classify   one wave per piece: frame header bytes + the sum over the piece's
//              chunks of 3 + Block_Size (a wave sum per 64 chunks, carried),
//              which is what the encoder's place kernel states as the frame's
//              size; the verdict from it.  No header byte is written.
//   fragments  one wave per extent: the totals over its pieces, and with
//              generate_fragments the run-length rows.  A piece starts a run
//              when it is the extent's first or its verdict differs from the
//              piece before (the neighbour lane's, the tile before's last one
//              carried); the run starts below a lane, counted from the ballot,
//              give the run its row.  A start writes its category and the bytes
//              before it; behind the last tile every row's bytes become the
//              distance to the next row's (the extent's end for the last one).
// The encoder's place and emit kernels are not launched: no frame is written
// and there is no output buffer.  No atomics.  Variable shifts are avoided
// ("64-bit shifts and the last VGPR"): lanes below are
// counted with mbcnt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RPP_LZ4_KERNEL_SIDE
#include "../lz4_internal.h"
#include "../zstd_enc_common.h"
#include "../zstd_enc_internal.h"
#include "ricepp_amd.h"

namespace {

using rpp_lz4::EncodeWs;

constexpr uint32_t kWave = 64;
constexpr uint32_t kTotals = RPP_INCOMPRESSIBLE_TOTALS;

__device__ inline uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

__device__ inline uint64_t wave_sum64(uint64_t v) {
  for (uint32_t d = kWave / 2; d; d >>= 1) v += uint64_t(__shfl_xor(static_cast<unsigned long long>(v), int(d)));
  return v;
}

__device__ inline uint64_t wave_incl_sum64(uint64_t v, uint32_t lane) {
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint64_t o = uint64_t(__shfl_up(static_cast<unsigned long long>(v), d));
    if (lane >= d) v += o;
  }
  return v;
}

// the set bits of `mask` below this lane
__device__ inline uint32_t bits_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}

// what this wave stored to global memory is read back by other lanes behind this
__device__ inline void wave_publish() {
  __threadfence();
  __syncthreads();
}

// ---------------------------------------------------------------------------
// classify: one wave per piece
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_incompressible_classify_kernel(const uint64_t* __restrict__ n_bytes,
                                                                           uint32_t npieces, EncodeWs ws,
                                                                           const uint32_t* __restrict__ block_size,
                                                                           const int32_t* __restrict__ status,
                                                                           double max_ratio, uint64_t* sizes,
                                                                           uint32_t* verdicts) {
  const uint32_t p = blockIdx.x, lane = lane_id();
  if (p >= npieces || !*ws.ok || status[p] != RPP_OK) return;  // (the prep kernel has zeroed size and verdict)
  const uint64_t n = n_bytes[p];
  const uint32_t g0 = ws.chunk_base[p], nc = ws.chunk_base[p + 1] - g0;
  uint8_t header[9];  // (stays in registers: only its size counts)
  uint64_t run = rpp_zstd::frame_header(n, header);
  for (uint32_t t = 0; t < nc; t += kWave) {
    const uint32_t c = t + lane;
    run += wave_sum64(c < nc ? 3 + block_size[g0 + c] : 0);
  }
  if (n == 0) run += 3;  // an empty frame has no chunk: its one block is an empty Raw block
  if (lane == 0) {
    sizes[p] = run;
    verdicts[p] = double(run) >= max_ratio * double(n) ? 1u : 0u;
  }
}

// ---------------------------------------------------------------------------
// fragments: one wave per extent
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_incompressible_fragments_kernel(
    const uint64_t* __restrict__ n_bytes, uint32_t npieces, const uint32_t* __restrict__ piece_base, uint32_t nextents,
    const uint64_t* __restrict__ sizes, const uint32_t* __restrict__ verdicts, double max_ratio,
    uint32_t generate_fragments, uint64_t* totals, uint64_t* frag_rows, uint32_t* frag_count) {
  const uint32_t e = blockIdx.x, lane = lane_id();
  if (e >= nextents) return;
  const uint32_t last = min(piece_base[e + 1], npieces), first = min(piece_base[e], last);
  uint64_t* const rows = frag_rows + 2 * uint64_t(first);
  uint64_t in_sum = 0, out_sum = 0, before = 0;  // per lane; per lane; the extent's bytes before the tile
  uint32_t hard = 0, count = 0, carry = 0;       // per lane; runs so far; the last verdict of the tile before
  for (uint32_t t = first; t < last; t += kWave) {
    const uint32_t i = t + lane, here = min(last - t, kWave);
    const bool has = i < last;
    const uint64_t n = has ? n_bytes[i] : 0;
    const uint32_t v = has ? verdicts[i] : 0;
    in_sum += n;
    out_sum += has ? sizes[i] : 0;
    hard += v;
    if (generate_fragments) {
      uint32_t prev = __shfl_up(v, 1);
      if (lane == 0) prev = carry;
      const bool start = has && (i == first || v != prev);
      const uint64_t starts = __ballot(start);
      const uint64_t incl = wave_incl_sum64(n, lane);
      if (start) {
        uint64_t* const row = rows + 2 * uint64_t(count + bits_below(starts));
        row[0] = v;
        row[1] = before + incl - n;
      }
      count += uint32_t(__popcll(starts));
      before += uint64_t(__shfl(static_cast<unsigned long long>(incl), int(kWave - 1)));
      carry = uint32_t(__shfl(v, int(here - 1)));
    }
  }
  const uint64_t total_in = wave_sum64(in_sum), total_out = wave_sum64(out_sum);
  const uint32_t blocks = last - first, hard_blocks = uint32_t(wave_sum64(hard));
  if (lane == 0) {
    uint64_t* const t = totals + uint64_t(e) * kTotals;
    t[0] = total_in;
    t[1] = total_out;
    t[2] = blocks;
    t[3] = hard_blocks;
    t[4] = blocks > 0 && double(total_out) >= max_ratio * double(total_in) ? 1 : 0;
    frag_count[e] = count;
  }
  if (count == 0) return;
  wave_publish();
  for (uint32_t t = 0; t < count; t += kWave) {  // a row's bytes: from where it starts to where the next one does
    const uint32_t k = t + lane;
    uint64_t from = 0, to = 0;
    if (k < count) {
      from = rows[2 * uint64_t(k) + 1];
      to = k + 1 < count ? rows[2 * uint64_t(k) + 3] : total_in;
    }
    __syncthreads();  // (row k + 1 is read before its lane stores; the next tile's first row is still a start)
    if (k < count) rows[2 * uint64_t(k) + 1] = to - from;
  }
}

uint64_t align16(uint64_t v) { return (v + 15) & ~UINT64_C(15); }

}  // namespace

extern "C" uint64_t rpp_incompressible_workspace_bytes(uint64_t total_bytes, uint32_t npieces, uint32_t nextents) {
  (void)nextents;  // (an extent needs no scratch: its rows and totals are the caller's)
  return align16(rpp_zstd_encode_workspace_bytes(total_bytes, npieces));
}

extern "C" uint64_t rpp_incompressible_workspace_bytes_long(uint64_t total_bytes, uint32_t npieces,
                                                            uint32_t nextents, uint32_t long_mode) {
  (void)nextents;
  return align16(rpp_zstd_encode_workspace_bytes_long(total_bytes, npieces, long_mode));
}

extern "C" int rpp_incompressible_scan_batch(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                             const uint64_t* d_in_bytes, uint32_t npieces,
                                             const uint32_t* d_piece_base, uint32_t nextents, double max_ratio,
                                             uint32_t generate_fragments, uint32_t options, uint32_t search,
                                             uint64_t* d_sizes, uint32_t* d_verdicts, uint64_t* d_totals,
                                             uint64_t* d_frag_rows, uint32_t* d_frag_count, int32_t* d_status,
                                             uint64_t total_bytes, void* d_workspace, uint64_t workspace_bytes,
                                             void* stream) {
  return rpp_incompressible_scan_batch_long(d_in, d_in_offsets, d_in_bytes, npieces, d_piece_base, nextents, max_ratio,
                                            generate_fragments, options, search, 0, d_sizes, d_verdicts, d_totals,
                                            d_frag_rows, d_frag_count, d_status, total_bytes, d_workspace,
                                            workspace_bytes, stream);
}

// ... under the Zstandard encoder's `long` word (0: the call above); the sizes are rpp_zstd_encode_batch_long's
extern "C" int rpp_incompressible_scan_batch_long(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                                  const uint64_t* d_in_bytes, uint32_t npieces,
                                                  const uint32_t* d_piece_base, uint32_t nextents, double max_ratio,
                                                  uint32_t generate_fragments, uint32_t options, uint32_t search,
                                                  uint32_t long_mode, uint64_t* d_sizes, uint32_t* d_verdicts,
                                                  uint64_t* d_totals, uint64_t* d_frag_rows, uint32_t* d_frag_count,
                                                  int32_t* d_status, uint64_t total_bytes, void* d_workspace,
                                                  uint64_t workspace_bytes, void* stream) {
  if ((options & ~rpp_zstd::kEncOptionsMask) || !rpp_lz4::search_valid(search) || long_mode > 1)
    return RPP_INVALID_ARGUMENT;
  if (npieces == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_sizes || !d_verdicts || !d_frag_rows || !d_status || !d_workspace ||
      ((uintptr_t)d_workspace & 15) || (nextents && (!d_piece_base || !d_totals || !d_frag_count)))
    return RPP_INVALID_ARGUMENT;
  if (rpp_lz4::max_chunks_of(total_bytes, npieces) >= 0x7fffffffu) return RPP_INVALID_ARGUMENT;
  if (workspace_bytes < rpp_incompressible_workspace_bytes_long(total_bytes, npieces, nextents, long_mode))
    return RPP_OUTPUT_TOO_SMALL;
  const rpp_zstd::EntropyStage st =
      rpp_zstd::launch_search_entropy(d_in, d_in_offsets, d_in_bytes, npieces, options, search, long_mode, d_sizes,
                                      d_verdicts, d_status, total_bytes, d_workspace, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_incompressible_classify_kernel, dim3(npieces), dim3(kWave), 0, s, d_in_bytes, npieces, st.ws,
                     st.block_size, d_status, max_ratio, d_sizes, d_verdicts);
  if (nextents)
    hipLaunchKernelGGL(rpp_incompressible_fragments_kernel, dim3(nextents), dim3(kWave), 0, s, d_in_bytes, npieces,
                       d_piece_base, nextents, d_sizes, d_verdicts, max_ratio, generate_fragments, d_totals,
                       d_frag_rows, d_frag_count);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}
