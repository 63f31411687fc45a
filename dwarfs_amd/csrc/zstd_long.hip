// zstd_long.hip -- the long-distance matcher of the Zstandard encoder on the
// GPU (gfx950), for the `long` word of rpp_zstd_encode_batch_long.  The
// definition is stated at the top of zstd_long_host.cpp, which holds the
// sequential restatement; the constants and the hash are in zstd_long_common.h.
//
// Four launches around the short search (lz4_internal.h), which does not change:
//   prepare  in front of the LZ4 prep kernel, one wave: per block the size that
//            every later kernel sees (a block above kLongMaxBlock gets a size
//            that the prep kernel refuses, so it has no chunks and nothing of
//            it is read) and where its table starts; the tables are cleared to
//            kLongEmpty behind it;
//   index    256 lanes per chunk, one lane per grid position: long_hash of the
//            window and an atomicMin of the position into the block's table.
//            The lowest position wins whatever the order, and it is a legal
//            source for every later occurrence;
//   find     one wave per chunk, in steps of 64 positions: every lane hashes
//            its window, looks the entry up and compares the kLongWindow bytes;
//            a ballot gives the hits, which are taken in order from the cursor
//            on; a hit is extended forward and backward by the whole wave, 64
//            bytes per turn, and kept from kLongMinMatch bytes on;
//   merge    one wave per chunk, behind the short search: the chunk's long
//            matches go to LDS, every short match finds by two binary searches
//            the first and the last long match that overlaps it and so its
//            parts (none, itself, head, tail, both); a prefix sum over the parts
//            and the count of long matches in front give every record its
//            place in the final list.  That list is a buffer of its own, so
//            nothing is read after it was overwritten; the entropy kernel gets
//            it in the short list's place.
// The windows are read from global memory as they are (unaligned 4-byte loads
// that neighbouring lanes share through the cache); the table lookups are
// random 4-byte loads.  Variable shifts are 32-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RPP_LZ4_KERNEL_SIDE
#include "lz4_internal.h"
#include "ricepp_amd.h"
#include "zstd_long_common.h"
#include "zstd_long_internal.h"

namespace {

using namespace rpp_zstd_long;
using rpp_lz4::block_of_chunk;
using rpp_lz4::EncodeWs;
using rpp_lz4::kChunk;
using rpp_lz4::kSeqsPerChunk;

constexpr uint32_t kWave = 64;
constexpr uint32_t kIndexLanes = 256;
constexpr uint64_t kRefused = rpp_lz4::kMaxBlock + 1;  // a size that the prep kernel refuses
constexpr uint32_t kHeadFlag = 0x8000u;
static_assert(kSeqsPerChunk < kHeadFlag, "a count of parts leaves the flag's bit free");
static_assert(kLongMaxBlock <= rpp_lz4::kMaxBlock, "a block the matcher takes is one the search takes");

__device__ inline uint32_t wave_incl_sum(uint32_t v, uint32_t lane) {
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ inline uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__global__ __launch_bounds__(kWave) void rpp_zstd_long_prepare_kernel(const uint64_t* __restrict__ n_bytes,
                                                                     uint32_t nblocks, LongWs lws) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint64_t running = 0;
  for (uint32_t base = 0; base < nblocks; base += kWave) {
    const uint32_t b = base + lane;
    uint32_t e = 0;
    if (b < nblocks) {
      const uint64_t n = n_bytes[b];
      const bool fits = n <= kLongMaxBlock;
      lws.n_eff[b] = fits ? n : kRefused;
      e = fits ? 1u << long_table_log(n) : 0;
    }
    const uint32_t incl = wave_incl_sum(e, lane);  // (64 tables of 2^23 entries at most: no overflow)
    if (b < nblocks) lws.tab_base[b] = running + incl - e;
    running += uint32_t(__shfl(incl, kWave - 1));
  }
  const bool ok = running <= lws.tab_entries;
  if (lane == 0) lws.tab_base[nblocks] = ok ? running : 0;
  if (!ok)  // the batch is larger than the caller promised: every block is refused
    for (uint32_t b = lane; b < nblocks; b += kWave) {
      lws.n_eff[b] = kRefused;
      lws.tab_base[b] = 0;
    }
}

struct ChunkView {
  const uint8_t* in;
  uint32_t* tab;
  uint32_t n, cs, ce, log;
};

__device__ inline ChunkView chunk_view(const uint8_t* d_in, const uint64_t* in_offsets, uint32_t nblocks,
                                       const EncodeWs& ws, const LongWs& lws, uint32_t g) {
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  ChunkView v;
  v.in = d_in + in_offsets[b];
  v.n = uint32_t(lws.n_eff[b]);  // (a block with chunks is no larger than kLongMaxBlock)
  v.cs = (g - ws.chunk_base[b]) * kChunk;
  v.ce = min(v.cs + kChunk, v.n);
  v.log = long_table_log(v.n);
  v.tab = lws.tab + lws.tab_base[b];
  return v;
}

__global__ __launch_bounds__(kIndexLanes) void rpp_zstd_long_index_kernel(const uint8_t* __restrict__ d_in,
                                                                         const uint64_t* __restrict__ in_offsets,
                                                                         uint32_t nblocks, EncodeWs ws, LongWs lws) {
  const uint32_t g = blockIdx.x;
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const ChunkView v = chunk_view(d_in, in_offsets, nblocks, ws, lws, g);
  for (uint32_t q = v.cs + kLongGrid * threadIdx.x; q < v.ce && q + kLongWindow <= v.n; q += kLongGrid * kIndexLanes) {
    uint32_t w[kLongWindow / 4];
#pragma unroll
    for (uint32_t k = 0; k < kLongWindow / 4; ++k) w[k] = rd32(v.in + q + 4 * k);
    atomicMin(&v.tab[long_slot(long_hash(w), v.log)], q);
  }
}

__global__ __launch_bounds__(kWave) void rpp_zstd_long_find_kernel(const uint8_t* __restrict__ d_in,
                                                                  const uint64_t* __restrict__ in_offsets,
                                                                  uint32_t nblocks, EncodeWs ws, LongWs lws) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x & (kWave - 1);
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const ChunkView v = chunk_view(d_in, in_offsets, nblocks, ws, lws, g);
  const uint8_t* const in = v.in;
  uint2* const out = lws.lseqs + uint64_t(g) * kLongPerChunk;
  uint32_t cnt = 0, cursor = v.cs;
  if (v.n >= kLongMinMatch + rpp_lz4::kLastLiterals) {
    const uint32_t lim_end = min(v.ce, v.n - rpp_lz4::kLastLiterals);
    for (uint32_t ss = v.cs; ss + kLongWindow <= lim_end; ss += kWave) {
      if (cursor >= ss + kWave) continue;
      const uint32_t p = ss + lane;
      bool hit = false;
      uint32_t q = 0;
      if (p >= cursor && p + kLongWindow <= lim_end) {  // (the cursor only grows: a lane behind it is never taken)
        uint32_t w[kLongWindow / 4];
#pragma unroll
        for (uint32_t k = 0; k < kLongWindow / 4; ++k) w[k] = rd32(in + p + 4 * k);
        q = v.tab[long_slot(long_hash(w), v.log)];
        if (q != kLongEmpty && q < p) {
          uint32_t x = 0;
#pragma unroll
          for (uint32_t k = 0; k < kLongWindow / 4; ++k) x |= rd32(in + q + 4 * k) ^ w[k];
          hit = x == 0;
        }
      }
      const uint64_t mask = __ballot(hit);
      uint32_t mask_lo = uint32_t(mask), mask_hi = uint32_t(mask >> 32);
      for (;;) {
        const uint32_t rel = max(cursor, ss) - ss;
        if (rel >= kWave) break;
        // the hits from `rel` on
        const uint32_t lo = rel < 32 ? mask_lo & (~0u << rel) : 0;
        const uint32_t hi = rel < 32 ? mask_hi : mask_hi & (~0u << (rel - 32));
        if (!(lo | hi)) break;
        const uint32_t l = lo ? uint32_t(__builtin_ctz(lo)) : 32 + uint32_t(__builtin_ctz(hi)), p0 = ss + l;
        const uint32_t q0 = uint32_t(__shfl(int(q), int(l)));
        const uint32_t lim = lim_end - p0, room = min(p0 - cursor, q0);
        uint32_t fwd = kLongWindow, back = 0;
        while (fwd < lim) {  // 64 bytes compared per turn
          const uint32_t k = fwd + lane;
          const uint64_t d = __ballot(k >= lim || in[q0 + k] != in[p0 + k]);
          if (d) {
            fwd += uint32_t(__builtin_ctzll(d));
            break;
          }
          fwd += kWave;
        }
        while (back < room) {
          const uint32_t k = back + lane;
          const uint64_t d = __ballot(k >= room || in[q0 - 1 - k] != in[p0 - 1 - k]);
          if (d) {
            back += uint32_t(__builtin_ctzll(d));
            break;
          }
          back += kWave;
        }
        if (fwd + back >= kLongMinMatch) {
          if (lane == 0 && cnt < kLongPerChunk)
            out[cnt] = make_uint2(rec_x(p0 - back - v.cs, p0 - q0), rec_y(fwd + back, p0 - q0));
          ++cnt;
          cursor = p0 + fwd;
        } else if (l < 32) {  // a candidate that is not kept changes nothing
          mask_lo &= ~(1u << l);
        } else {
          mask_hi &= ~(1u << (l - 32));
        }
      }
    }
  }
  if (lane == 0) lws.lcnt[g] = min(cnt, kLongPerChunk);  // (matches of 64 bytes that do not overlap: never more)
}

struct Parts {  // of a short match [a, b) among the chunk's long matches
  uint32_t f, l;  // the first long match that ends behind a; the last one that starts before b
  bool overlap, head, tail;
};

__device__ inline Parts classify(const uint32_t* lpos, const uint32_t* lend, uint32_t nl, uint32_t a, uint32_t b) {
  uint32_t lo = 0, hi = nl;
  while (lo < hi) {  // the first j with lend[j] > a
    const uint32_t mid = (lo + hi) / 2;
    if (lend[mid] > a) hi = mid; else lo = mid + 1;
  }
  Parts r;
  r.f = lo;
  r.overlap = lo < nl && lpos[lo] < b;
  r.l = lo;
  r.head = r.tail = false;
  if (r.overlap) {
    hi = nl;
    while (lo < hi) {  // the first j with lpos[j] >= b
      const uint32_t mid = (lo + hi) / 2;
      if (lpos[mid] >= b) hi = mid; else lo = mid + 1;
    }
    r.l = lo - 1;
    r.head = lpos[r.f] >= a + rpp_lz4::kMinMatch;
    r.tail = lend[r.l] + rpp_lz4::kMinMatch <= b;
  }
  return r;
}

__global__ __launch_bounds__(kWave) void rpp_zstd_long_merge_kernel(uint32_t nblocks, EncodeWs ws, LongWs lws) {
  __shared__ uint32_t lpos[kLongPerChunk], lend[kLongPerChunk];
  __shared__ uint16_t pre[kSeqsPerChunk];  // per short match: parts in front of its own | kHeadFlag
  const uint32_t g = blockIdx.x, lane = threadIdx.x & (kWave - 1);
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t nl = min(lws.lcnt[g], kLongPerChunk), ns = min(ws.cnt[g], kSeqsPerChunk);
  const uint2* const sh = ws.seqs + uint64_t(g) * kSeqsPerChunk;
  const uint2* const lg = lws.lseqs + uint64_t(g) * kLongPerChunk;
  uint2* const out = lws.mseqs + uint64_t(g) * kSeqsPerChunk;
  for (uint32_t j = lane; j < nl; j += kWave) {
    const uint2 r = lg[j];
    lpos[j] = rec_rel(r.x);
    lend[j] = rec_rel(r.x) + rec_len(r.y);
  }
  __syncthreads();
  uint32_t total = 0;  // the short matches' parts
  for (uint32_t t = 0; t < ns; t += kWave) {
    const uint32_t i = t + lane;
    uint32_t parts = 0, head = 0;
    if (i < ns) {
      const uint2 s = sh[i];
      const Parts r = classify(lpos, lend, nl, rec_rel(s.x), rec_rel(s.x) + rec_len(s.y));
      parts = r.overlap ? uint32_t(r.head) + uint32_t(r.tail) : 1;
      head = r.head ? kHeadFlag : 0;
    }
    const uint32_t incl = wave_incl_sum(parts, lane);
    if (i < ns) pre[i] = uint16_t((total + incl - parts) | head);
    total += uint32_t(__shfl(incl, kWave - 1));
  }
  __syncthreads();
  // A part at x stands behind the parts in front of it and the long matches that start before x; the list holds
  // at most kSeqsPerChunk records (they do not overlap and have at least kMinMatch bytes).
  for (uint32_t t = 0; t < ns; t += kWave) {
    const uint32_t i = t + lane;
    if (i >= ns) continue;
    const uint2 s = sh[i];
    const uint32_t a = rec_rel(s.x), b = a + rec_len(s.y), off = rec_off(s.x, s.y), base = pre[i] & (kHeadFlag - 1);
    const Parts r = classify(lpos, lend, nl, a, b);
    if (!r.overlap) {
      if (base + r.f < kSeqsPerChunk) out[base + r.f] = s;
      continue;
    }
    if (r.head && base + r.f < kSeqsPerChunk) out[base + r.f] = make_uint2(rec_x(a, off), rec_y(lpos[r.f] - a, off));
    const uint32_t at = base + uint32_t(r.head) + r.l + 1;
    if (r.tail && at < kSeqsPerChunk) out[at] = make_uint2(rec_x(lend[r.l], off), rec_y(b - lend[r.l], off));
  }
  for (uint32_t j = lane; j < nl; j += kWave) {
    const uint32_t x = lpos[j];
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {  // the first short match that ends behind x
      const uint32_t mid = (lo + hi) / 2;
      const uint2 s = sh[mid];
      if (rec_rel(s.x) + rec_len(s.y) > x) hi = mid; else lo = mid + 1;
    }
    uint32_t front = total;
    if (lo < ns) {  // its head, where it has one, stands in front as well
      const uint32_t e = pre[lo];
      front = (e & (kHeadFlag - 1)) + ((e & kHeadFlag) && rec_rel(sh[lo].x) < x ? 1u : 0u);
    }
    if (j + front < kSeqsPerChunk) out[j + front] = lg[j];
  }
  if (lane == 0) lws.mcnt[g] = min(total + nl, kSeqsPerChunk);
}

uint64_t align16(uint64_t v) { return (v + 15) & ~UINT64_C(15); }

}  // namespace

uint64_t rpp_zstd_long::workspace_bytes(uint64_t total_bytes, uint32_t nblocks) {
  const uint64_t mc = rpp_lz4::max_chunks_of(total_bytes, nblocks);
  return align16(8ull * nblocks) + align16(8ull * (nblocks + 1)) + align16(4 * long_table_entries(total_bytes, nblocks)) +
         2 * align16(4 * mc) + mc * (kLongPerChunk + kSeqsPerChunk) * sizeof(uint2);
}

rpp_zstd_long::LongWs rpp_zstd_long::carve(void* d, uint64_t total_bytes, uint32_t nblocks) {
  const uint64_t mc = rpp_lz4::max_chunks_of(total_bytes, nblocks);
  uint8_t* p = static_cast<uint8_t*>(d);
  auto take = [&p](uint64_t bytes) {
    uint8_t* r = p;
    p += align16(bytes);
    return r;
  };
  LongWs w{};
  w.tab_entries = long_table_entries(total_bytes, nblocks);
  w.n_eff = reinterpret_cast<uint64_t*>(take(8ull * nblocks));
  w.tab_base = reinterpret_cast<uint64_t*>(take(8ull * (nblocks + 1)));
  w.tab = reinterpret_cast<uint32_t*>(take(4 * w.tab_entries));
  w.lcnt = reinterpret_cast<uint32_t*>(take(4 * mc));
  w.mcnt = reinterpret_cast<uint32_t*>(take(4 * mc));
  w.lseqs = reinterpret_cast<uint2*>(take(mc * kLongPerChunk * sizeof(uint2)));
  w.mseqs = reinterpret_cast<uint2*>(take(mc * kSeqsPerChunk * sizeof(uint2)));
  return w;
}

void rpp_zstd_long::launch_prepare(const uint64_t* d_in_bytes, uint32_t nblocks, const LongWs& lws, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_zstd_long_prepare_kernel, dim3(1), dim3(kWave), 0, s, d_in_bytes, nblocks, lws);
  (void)hipMemsetAsync(lws.tab, 0xff, 4 * lws.tab_entries, s);  // kLongEmpty (an error shows in hipGetLastError)
}

void rpp_zstd_long::launch_match(const uint8_t* d_in, const uint64_t* d_in_offsets, uint32_t nblocks,
                                 const EncodeWs& ws, const LongWs& lws, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_zstd_long_index_kernel, dim3(ws.max_chunks), dim3(kIndexLanes), 0, s, d_in, d_in_offsets,
                     nblocks, ws, lws);
  hipLaunchKernelGGL(rpp_zstd_long_find_kernel, dim3(ws.max_chunks), dim3(kWave), 0, s, d_in, d_in_offsets, nblocks, ws,
                     lws);
  hipLaunchKernelGGL(rpp_zstd_long_merge_kernel, dim3(ws.max_chunks), dim3(kWave), 0, s, nblocks, ws, lws);
}
