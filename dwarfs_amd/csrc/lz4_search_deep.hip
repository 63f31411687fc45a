// lz4_search_deep.hip -- the deeper match search of the LZ4 and Zstandard
// encoders (gfx950): rpp_lz4_deep_search_kernel<DEPTH, LAZY>, one wave per
// 32 KiB chunk, in the place of rpp_lz4_search_kernel (lz4_kernels.hip) for a
// search word other than 0.  The definition is stated at the top of
// lz4_host.cpp, which holds the sequential restatement (find_sequences with a
// search word); the constants are in lz4_common.h.  It fills the same EncodeWs
// records, so the place, entropy and emit kernels behind it do not change.
//
// A hash value's bucket is DEPTH 16-bit entries in LDS, highest position first:
// position - window start + 1, 0 for none (the window is the kChunk bytes
// before the chunk; the chunk's last step is never inserted, nothing looks it
// up, so the highest entry is 2 * kChunk - kStep).  A step of 64 positions:
//   lookup   every lane reads its whole bucket in one LDS load;
//   insert   the lanes that share a hash find each other with one ballot per
//            hash bit, rank themselves by lane, and the DEPTH highest write
//            their slots; the highest also moves the old entries down.  Every
//            slot has one writer: no atomics, no rewriting;
//   score    every lane compares its own candidates, 4 bytes per load, up to
//            kDeepCap bytes each, all lanes at once;
//   choice   one ballot (LAZY: of the lanes whose right neighbour does not
//            score higher); serial over the matches taken, as in the greedy
//            kernel, and only a match that scored kDeepCap is extended by the
//            whole wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_common.h"
#define RPP_LZ4_KERNEL_SIDE
#include "lz4_internal.h"
#include "ricepp_amd.h"

namespace {

using namespace rpp_lz4;

constexpr uint32_t kWave = 64;
static_assert(kStep == kWave, "a search step is one wave of positions");
static_assert(2 * kChunk <= 65536, "window and chunk positions fit a 16-bit entry");
static_assert(kDeepCap >= kMinMatch && kDeepCap % 4 == 0, "the score loop compares 4 bytes per turn");

template <uint32_t DEPTH>
struct alignas(2 * DEPTH) Bucket {
  uint16_t e[DEPTH];
};

__device__ inline uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// The step's inserts: `v` goes into the bucket of `h` for every valid lane; `old` is that bucket as the lane
// read it before the step.  The bucket then holds the DEPTH highest of the old entries and the step's new ones
// (every new one lies above every old one, and a higher lane holds a higher position).
template <uint32_t DEPTH>
__device__ inline void insert_step(Bucket<DEPTH>* tab, bool valid, uint32_t h, uint32_t v, const Bucket<DEPTH>& old) {
  uint64_t same = __ballot(valid);  // the valid lanes with this lane's hash
  for (uint32_t bit = 0; bit < kHashBits; ++bit) {
    const bool set = h >> bit & 1;
    const uint64_t b = __ballot(set);
    same &= set ? b : ~b;
  }
  if (valid) {
    const uint32_t lo = uint32_t(same), hi = uint32_t(same >> 32);
    const uint32_t m = uint32_t(__builtin_popcount(lo) + __builtin_popcount(hi));
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0));
    const uint32_t rank = m - 1 - below;  // lanes of the same hash above this one
    if (rank < DEPTH) tab[h].e[rank] = uint16_t(v);
    if (rank == 0) {
#pragma unroll
      for (uint32_t k = 0; k < DEPTH; ++k)
        if (k + m < DEPTH) tab[h].e[k + m] = old.e[k];
    }
  }
}

template <uint32_t DEPTH, bool LAZY>
__global__ __launch_bounds__(kWave) void rpp_lz4_deep_search_kernel(const uint8_t* __restrict__ d_in,
                                                                   const uint64_t* __restrict__ in_offsets,
                                                                   const uint64_t* __restrict__ n_bytes,
                                                                   uint32_t nblocks, EncodeWs ws) {
  __shared__ __attribute__((aligned(16))) Bucket<DEPTH> tab[1u << kHashBits];  // 8 KiB * DEPTH
  const uint32_t g = blockIdx.x, lane = threadIdx.x & (kWave - 1);
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  const uint8_t* const in = d_in + in_offsets[b];
  const uint32_t n = uint32_t(n_bytes[b]);
  const uint32_t cs = (g - ws.chunk_base[b]) * kChunk, ce = min(cs + kChunk, n);
  uint32_t cnt = 0, first_pos = 0, body = 0, cursor = cs;
  if (n >= kMatchStartGap + 1) {
    const uint32_t last_start = n - kMatchStartGap, lim_end = min(ce, n - kLastLiterals);
    const uint32_t w0 = cs >= kChunk ? cs - kChunk : 0;  // the window's start
    uint32_t* const words = reinterpret_cast<uint32_t*>(tab);
    for (uint32_t i = lane; i < (DEPTH << kHashBits) / 2; i += kWave) words[i] = 0;
    __syncthreads();
    for (uint32_t q0 = w0; q0 < cs; q0 += kWave) {
      const uint32_t q = q0 + lane;
      const bool valid = q < cs && q + 4 <= n;
      const uint32_t h = valid ? hash4(rd32(in + q)) : 0;
      const Bucket<DEPTH> old = tab[h];
      __syncthreads();
      insert_step<DEPTH>(tab, valid, h, q - w0 + 1, old);
      __syncthreads();
    }
    uint2* const seqs = ws.seqs + uint64_t(g) * kSeqsPerChunk;
    for (uint32_t ss = cs; ss < ce; ss += kStep) {
      const uint32_t se = min(ss + kStep, ce);
      if (cursor >= se) continue;
      const uint32_t p = ss + lane;
      const bool valid = p < se && p + 4 <= n;
      const uint32_t word = valid ? rd32(in + p) : 0, h = valid ? hash4(word) : 0;
      const Bucket<DEPTH> old = tab[h];
      __syncthreads();  // every lookup of the step precedes its inserts
      if (ss + kStep < ce) {  // (nothing looks up what the chunk's last step would insert)
        insert_step<DEPTH>(tab, valid, h, p - w0 + 1, old);
        __syncthreads();
      }
      uint32_t best = 0, score = 0;  // best: the entry of the candidate; 0: none
      if (valid && p >= cursor && p <= last_start && p + 4 <= lim_end) {
        const uint32_t cap = min(lim_end - p, kDeepCap);
#pragma unroll
        for (uint32_t k = 0; k < DEPTH; ++k) {
          const uint32_t e = old.e[k];
          if (e == 0) break;
          const uint8_t* const c = in + (w0 + e - 1);
          if (p - (w0 + e - 1) > kMaxOffset || rd32(c) != word) continue;
          uint32_t s = kMinMatch;
          bool open = true;  // no differing byte seen
          while (s + 4 <= cap) {
            const uint32_t x = rd32(c + s) ^ rd32(in + p + s);
            if (x) {
              s += uint32_t(__builtin_ctz(x)) >> 3;
              open = false;
              break;
            }
            s += 4;
          }
          if (open)
            while (s < cap && c[s] == in[p + s]) ++s;
          if (s > score) {  // (of equal scores the first, which is the highest position)
            score = s;
            best = e;
          }
        }
      }
      bool take = best != 0;
      if (LAZY) {
        const uint32_t next = uint32_t(__shfl_down(int(score), 1));  // (0 where p + 1 has no best)
        take = take && !(lane + 1 < kWave && next > score);
      }
      const uint64_t mask = __ballot(take);
      const uint32_t mask_lo = uint32_t(mask), mask_hi = uint32_t(mask >> 32);
      for (;;) {
        const uint32_t rel = max(cursor, ss) - ss;
        if (rel >= kStep) break;
        // the lanes from `rel` on (32-bit shifts: DESIGN.md section 4)
        const uint32_t lo = rel < 32 ? mask_lo & (~0u << rel) : 0;
        const uint32_t hi = rel < 32 ? mask_hi : mask_hi & (~0u << (rel - 32));
        if (!(lo | hi)) break;
        const uint32_t l = lo ? uint32_t(__builtin_ctz(lo)) : 32 + uint32_t(__builtin_ctz(hi)), p0 = ss + l;
        const uint32_t c0 = w0 + uint32_t(__shfl(int(best), int(l))) - 1;
        const uint32_t lim = lim_end - p0;
        uint32_t len = uint32_t(__shfl(int(score), int(l)));
        if (len == kDeepCap)  // (a lower score is the whole common prefix)
          while (len < lim) {  // 64 bytes compared per turn
            const uint32_t k = len + lane;
            const bool differs = k >= lim || in[c0 + k] != in[p0 + k];
            const uint64_t d = __ballot(differs);
            if (d) {
              len += uint32_t(__builtin_ctzll(d));
              break;
            }
            len += kWave;
          }
        if (lane == 0) seqs[cnt] = make_uint2((p0 - cs) | (p0 - c0) << 16, len);
        if (cnt == 0) {
          first_pos = p0;
          body += 3 + ext_bytes(len - kMinMatch);
        } else {
          body += seq_bytes(p0 - cursor, len);
        }
        ++cnt;
        cursor = p0 + len;
      }
    }
  }
  if (lane == 0) {
    ws.cnt[g] = cnt;
    ws.first_pos[g] = first_pos;
    ws.last_end[g] = cnt ? cursor : 0;
    ws.body[g] = body;
  }
}

template <uint32_t DEPTH>
void launch(bool lazy, hipStream_t s, const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
            uint32_t nblocks, const EncodeWs& ws) {
  if (lazy)
    hipLaunchKernelGGL((rpp_lz4_deep_search_kernel<DEPTH, true>), dim3(ws.max_chunks), dim3(kWave), 0, s, d_in,
                       d_in_offsets, d_in_bytes, nblocks, ws);
  else
    hipLaunchKernelGGL((rpp_lz4_deep_search_kernel<DEPTH, false>), dim3(ws.max_chunks), dim3(kWave), 0, s, d_in,
                       d_in_offsets, d_in_bytes, nblocks, ws);
}

}  // namespace

void rpp_lz4::launch_deep_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                 uint32_t nblocks, const EncodeWs& ws, uint32_t search, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool lazy = search & kSearchLazy;
  switch (search & ~kSearchLazy) {
    case 1: return launch<1>(lazy, s, d_in, d_in_offsets, d_in_bytes, nblocks, ws);
    case 2: return launch<2>(lazy, s, d_in, d_in_offsets, d_in_bytes, nblocks, ws);
    case 4: return launch<4>(lazy, s, d_in, d_in_offsets, d_in_bytes, nblocks, ws);
    default: return launch<8>(lazy, s, d_in, d_in_offsets, d_in_bytes, nblocks, ws);
  }
}
