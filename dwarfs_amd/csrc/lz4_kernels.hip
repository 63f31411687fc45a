// lz4_kernels.hip -- the LZ4 block codec on the GPU (gfx950): one wave per
// stream for decode, one wave per 32 KiB chunk for the encoder's match search
// and emission.  The contracts, the malformed-input rules and the encoder's
// deterministic definition are stated at the top of lz4_host.cpp, which holds
// the sequential restatement of both; the constants are in lz4_common.h.
//
// Decode reads a match back through global memory.  The bytes were stored by
// the same wave, so one `s_waitcnt vmcnt(0)` between the stores and the loads
// is enough: a wave's stores are complete once the counter has drained, and the
// loads that follow go through the same CU's vector L1, which is write-through
// and coherent for its own CU.  The wait is taken only when a match reaches
// into bytes stored since the last wait (a watermark).  Every match is copied
// from bytes that precede it: destination byte j is source byte j mod offset,
// so the steps of one copy never depend on each other.  An LDS window of 64 KiB
// would leave two waves per CU; this leaves occupancy to hide the latency.
//
// The encoder has no atomics: a table entry contested inside one step is
// settled by rewriting until the highest position stands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lz4_common.h"
#define RPP_LZ4_KERNEL_SIDE
#include "lz4_internal.h"
#include "ricepp_amd.h"

namespace {

using namespace rpp_lz4;

constexpr uint32_t kWave = 64;
constexpr uint32_t kDecodeWaves = 4;  // streams per decode workgroup
static_assert(kStep == kWave, "a search step is one wave of positions");

__device__ inline uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

__device__ inline uint32_t rd32(const uint8_t* p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

__device__ inline uint32_t wave_incl_sum(uint32_t v, uint32_t lane) {
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ inline uint32_t wave_incl_max(uint32_t v, uint32_t lane) {
  for (uint32_t d = 1; d < kWave; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d && o > v) v = o;
  }
  return v;
}

// n bytes from s to d, the two ranges apart; 4 bytes per lane while 256 are left
__device__ inline void wave_copy(uint8_t* d, const uint8_t* s, uint64_t n, uint32_t lane) {
  uint64_t k = 0;
  for (; k + 256 <= n; k += 256) {
    uint32_t v;
    __builtin_memcpy(&v, s + k + 4 * lane, 4);
    __builtin_memcpy(d + k + 4 * lane, &v, 4);
  }
  for (uint64_t j = k + lane; j < n; j += kWave) d[j] = s[j];
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
struct Window {  // 64 bytes of the stream in the wave's registers: byte win + lane in lane `lane`
  const uint8_t* src;
  uint64_t in_n, win;
  uint32_t reg;
  bool loaded;
};

__device__ inline uint32_t peek(Window& w, uint64_t ip, uint32_t lane) {  // ip < in_n
  if (!w.loaded || ip < w.win || ip - w.win >= kWave) {
    w.win = ip;
    w.reg = ip + lane < w.in_n ? w.src[ip + lane] : 0;
    w.loaded = true;
  }
  return __shfl(w.reg, int(ip - w.win));
}

__global__ __launch_bounds__(kWave* kDecodeWaves) void rpp_lz4_decode_kernel(
    const uint8_t* __restrict__ d_in, const uint64_t* __restrict__ in_offsets, const uint64_t* __restrict__ in_bytes,
    uint32_t nblocks, uint8_t* d_out, const uint64_t* __restrict__ out_offsets,
    const uint64_t* __restrict__ out_bytes, int32_t* __restrict__ d_status) {
  const uint32_t b = blockIdx.x * kDecodeWaves + threadIdx.x / kWave, lane = lane_id();
  if (b >= nblocks) return;
  const uint64_t in_n = in_bytes[b], out_n = out_bytes[b];
  uint8_t* const dst = d_out + out_offsets[b];
  Window w{d_in + in_offsets[b], in_n, 0, 0, false};
  uint64_t ip = 0, op = 0, flushed = 0;  // flushed: output below it was stored before the last wait
  int32_t st = RPP_CORRUPT_INPUT;
  for (;;) {  // every turn consumes at least one byte of the stream
    if (ip >= in_n) break;
    const uint32_t token = peek(w, ip++, lane);
    uint64_t lit = token >> 4;
    bool bad = false;
    if (lit == 15)
      for (;;) {
        if (ip >= in_n) { bad = true; break; }
        const uint32_t x = peek(w, ip++, lane);
        lit += x;
        if (x != 255) break;
      }
    if (bad || lit > in_n - ip || lit > out_n - op) break;
    if (lit) {
      if (w.loaded && ip >= w.win && ip - w.win + lit <= kWave) {  // the literals are in the window
        const uint32_t v = __shfl(w.reg, int((ip - w.win + lane) & (kWave - 1)));
        if (lane < lit) dst[op + lane] = uint8_t(v);
      } else {
        wave_copy(dst + op, w.src + ip, lit, lane);
      }
    }
    ip += lit;
    op += lit;
    if (ip == in_n) { st = op == out_n ? RPP_OK : RPP_CORRUPT_INPUT; break; }
    if (in_n - ip < 2) break;
    const uint32_t lo = peek(w, ip, lane), hi = peek(w, ip + 1, lane);
    const uint32_t off = lo | hi << 8;
    ip += 2;
    if (off == 0 || off > op) break;
    uint64_t len = (token & 15) + kMinMatch;
    if ((token & 15) == 15)
      for (;;) {
        if (ip >= in_n) { bad = true; break; }
        const uint32_t x = peek(w, ip++, lane);
        len += x;
        if (x != 255) break;
      }
    if (bad || len > out_n - op) break;
    const uint8_t* const from = dst + op - off;
    const uint64_t span = len < off ? len : off;  // the source bytes the match reads
    if (op - off + span > flushed) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have landed
      flushed = op;
    }
    if (off >= len) {
      wave_copy(dst + op, from, len, lane);
    } else {  // a pattern of `off` bytes repeated
      uint32_t r = lane % off;
      const uint32_t adv = kWave % off;
      for (uint64_t j = lane; j < len; j += kWave) {
        dst[op + j] = from[r];
        r += adv;
        if (r >= off) r -= off;
      }
    }
    op += len;
  }
  if (lane == 0) d_status[b] = st;
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_lz4_prep_kernel(const uint64_t* __restrict__ n_bytes, uint32_t nblocks,
                                                            EncodeWs ws, uint64_t* out_bytes, uint32_t* flags,
                                                            int32_t* status) {
  const uint32_t lane = lane_id();
  uint64_t running = 0;
  for (uint32_t base = 0; base < nblocks; base += kWave) {
    const uint32_t b = base + lane;
    uint32_t c = 0;
    if (b < nblocks) {
      const uint64_t n = n_bytes[b];
      const bool fits = n <= kMaxBlock;
      status[b] = fits ? RPP_OK : RPP_INVALID_ARGUMENT;
      out_bytes[b] = 0;
      flags[b] = 0;
      c = fits ? uint32_t((n + kChunk - 1) / kChunk) : 0;
    }
    const uint32_t incl = wave_incl_sum(c, lane);  // (64 blocks of 2^15 chunks at most: no overflow)
    const uint64_t start = running + incl - c;
    if (b < nblocks) ws.chunk_base[b] = start > ws.max_chunks ? ws.max_chunks + 1 : uint32_t(start);
    running += __shfl(incl, kWave - 1);
  }
  const bool ok = running <= ws.max_chunks;
  if (lane == 0) {
    ws.chunk_base[nblocks] = ok ? uint32_t(running) : 0;
    *ws.ok = ok ? 1 : 0;
  }
  if (!ok)  // the batch is larger than the caller promised: nothing is encoded
    for (uint32_t b = lane; b < nblocks; b += kWave) status[b] = RPP_INVALID_ARGUMENT;
}

// table entries hold position + 1; the highest value offered for a slot stands
__device__ inline void insert_max(uint32_t* tab, bool valid, uint32_t h, uint32_t v) {
  bool pend = valid;
  while (__ballot(pend)) {  // at most one turn per lane that shares a slot
    if (pend && tab[h] < v) tab[h] = v;
    __syncthreads();
    pend = pend && tab[h] < v;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWave) void rpp_lz4_search_kernel(const uint8_t* __restrict__ d_in,
                                                              const uint64_t* __restrict__ in_offsets,
                                                              const uint64_t* __restrict__ n_bytes, uint32_t nblocks,
                                                              EncodeWs ws) {
  __shared__ uint32_t tab[1u << kHashBits];
  const uint32_t g = blockIdx.x, lane = lane_id();
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  const uint8_t* const in = d_in + in_offsets[b];
  const uint32_t n = uint32_t(n_bytes[b]);
  const uint32_t cs = (g - ws.chunk_base[b]) * kChunk, ce = min(cs + kChunk, n);
  uint32_t cnt = 0, first_pos = 0, body = 0, cursor = cs;
  if (n >= kMatchStartGap + 1) {
    const uint32_t last_start = n - kMatchStartGap, lim_end = min(ce, n - kLastLiterals);
    for (uint32_t i = lane; i < (1u << kHashBits); i += kWave) tab[i] = 0;
    __syncthreads();
    for (uint32_t q0 = cs >= kChunk ? cs - kChunk : 0; q0 < cs; q0 += kWave) {
      const uint32_t q = q0 + lane;
      const bool valid = q < cs && q + 4 <= n;
      insert_max(tab, valid, valid ? hash4(rd32(in + q)) : 0, q + 1);
    }
    uint2* const seqs = ws.seqs + uint64_t(g) * kSeqsPerChunk;
    for (uint32_t ss = cs; ss < ce; ss += kStep) {
      const uint32_t se = min(ss + kStep, ce);
      if (cursor >= se) continue;
      const uint32_t p = ss + lane;
      const bool valid = p < se && p + 4 <= n;
      const uint32_t word = valid ? rd32(in + p) : 0, h = hash4(word);
      const uint32_t cand = valid ? tab[h] : 0;
      __syncthreads();  // every lookup of the step precedes its inserts
      insert_max(tab, valid, h, p + 1);
      const bool has = cand != 0 && p <= last_start && p + 4 <= lim_end && p - (cand - 1) <= kMaxOffset &&
                       rd32(in + (cand - 1)) == word;
      const uint64_t mask = __ballot(has);
      const uint32_t mask_lo = uint32_t(mask), mask_hi = uint32_t(mask >> 32);
      for (;;) {
        const uint32_t rel = max(cursor, ss) - ss;
        if (rel >= kStep) break;
        // the lanes from `rel` on (32-bit shifts: DESIGN.md section 4)
        const uint32_t lo = rel < 32 ? mask_lo & (~0u << rel) : 0;
        const uint32_t hi = rel < 32 ? mask_hi : mask_hi & (~0u << (rel - 32));
        if (!(lo | hi)) break;
        const uint32_t l = lo ? uint32_t(__builtin_ctz(lo)) : 32 + uint32_t(__builtin_ctz(hi)), p0 = ss + l;
        const uint32_t c0 = uint32_t(__shfl(cand, int(l))) - 1;
        const uint32_t lim = lim_end - p0;
        uint32_t len = kMinMatch;
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

// one wave per block: where every chunk's sequences go, the block's size and its ratio flag
__global__ __launch_bounds__(kWave) void rpp_lz4_place_kernel(const uint64_t* __restrict__ n_bytes, uint32_t nblocks,
                                                             EncodeWs ws, uint8_t* d_out,
                                                             const uint64_t* __restrict__ out_offsets,
                                                             uint64_t* out_bytes, uint32_t* flags,
                                                             const int32_t* __restrict__ status) {
  const uint32_t b = blockIdx.x, lane = lane_id();
  if (!*ws.ok || status[b] != RPP_OK) return;
  const uint32_t n = uint32_t(n_bytes[b]);
  const uint32_t g0 = ws.chunk_base[b], nc = ws.chunk_base[b + 1] - g0;
  uint32_t carry_run = 0, off_run = 0;
  for (uint32_t t = 0; t < nc; t += kWave) {
    const uint32_t c = t + lane;
    const bool in_block = c < nc;
    const uint32_t cnt = in_block ? ws.cnt[g0 + c] : 0;
    const uint32_t le = cnt ? ws.last_end[g0 + c] : 0;
    const uint32_t incl_max = wave_incl_max(le, lane);
    uint32_t before = __shfl_up(incl_max, 1);
    if (lane == 0) before = 0;
    const uint32_t carry = max(carry_run, before);
    uint32_t size = 0;
    if (cnt) {
      const uint32_t lit = ws.first_pos[g0 + c] - carry;
      size = ws.body[g0 + c] + lit + ext_bytes(lit);
    }
    const uint32_t incl = wave_incl_sum(size, lane);
    if (in_block) {
      ws.carry[g0 + c] = carry;
      ws.out_off[g0 + c] = off_run + incl - size;
    }
    carry_run = max(carry_run, uint32_t(__shfl(incl_max, kWave - 1)));
    off_run += uint32_t(__shfl(incl, kWave - 1));
  }
  if (lane == 0) {
    const uint32_t lit = n - carry_run;
    const uint64_t total = uint64_t(off_run) + 1 + ext_bytes(lit) + lit;
    ws.fin_anchor[b] = carry_run;
    ws.fin_off[b] = off_run;
    out_bytes[b] = total;
    flags[b] = 4 + total >= n ? 1u : 0u;
    if (n == 0) d_out[out_offsets[b]] = 0;  // an empty block has no chunk to emit its one token
  }
}

// `v` >= 15 behind a nibble: 255s, then the rest
__device__ inline uint32_t wave_put_length(uint8_t* o, uint32_t v, uint32_t lane) {
  const uint32_t r = v - 15, nb = r / 255 + 1;
  for (uint32_t k = lane; k < nb; k += kWave) o[k] = k + 1 == nb ? uint8_t(r % 255) : uint8_t(255);
  return nb;
}

// one sequence by the whole wave; len == 0: the block's last literal run
__device__ inline void wave_emit(uint8_t* o, const uint8_t* lits, uint32_t lit, uint32_t len, uint32_t off,
                                 uint32_t lane) {
  const uint32_t ml = len ? len - kMinMatch : 0;
  if (lane == 0) o[0] = uint8_t(min(lit, 15u) << 4 | min(ml, 15u));
  uint32_t at = 1;
  if (lit >= 15) at += wave_put_length(o + at, lit, lane);
  wave_copy(o + at, lits, lit, lane);
  at += lit;
  if (len) {
    if (lane == 0) {
      o[at] = uint8_t(off);
      o[at + 1] = uint8_t(off >> 8);
    }
    if (ml >= 15) wave_put_length(o + at + 2, ml, lane);
  }
}

__global__ __launch_bounds__(kWave) void rpp_lz4_emit_kernel(const uint8_t* __restrict__ d_in,
                                                            const uint64_t* __restrict__ in_offsets,
                                                            const uint64_t* __restrict__ n_bytes, uint32_t nblocks,
                                                            EncodeWs ws, uint8_t* __restrict__ d_out,
                                                            const uint64_t* __restrict__ out_offsets) {
  const uint32_t g = blockIdx.x, lane = lane_id();
  if (!*ws.ok || g >= ws.chunk_base[nblocks]) return;
  const uint32_t b = block_of_chunk(ws.chunk_base, nblocks, g);
  const uint8_t* const in = d_in + in_offsets[b];
  uint8_t* const out = d_out + out_offsets[b];
  const uint32_t n = uint32_t(n_bytes[b]);
  const uint32_t c = g - ws.chunk_base[b], cs = c * kChunk;
  const uint32_t cnt = ws.cnt[g];
  const uint2* const seqs = ws.seqs + uint64_t(g) * kSeqsPerChunk;
  uint32_t prev_end = ws.carry[g], o = ws.out_off[g];
  for (uint32_t t = 0; t < cnt; t += kWave) {
    const uint32_t i = t + lane, here = min(cnt - t, kWave);
    const bool has = i < cnt;
    const uint2 s = has ? seqs[i] : make_uint2(0, 0);
    const uint32_t pos = cs + (s.x & 0xffffu), len = s.y, off = s.x >> 16;
    const uint32_t end = has ? pos + len : 0;
    uint32_t prev = __shfl_up(end, 1);
    if (lane == 0) prev = prev_end;
    const uint32_t lit = has ? pos - prev : 0;
    const uint32_t size = has ? seq_bytes(lit, len) : 0;
    const uint32_t incl = wave_incl_sum(size, lane);
    const uint32_t mine = o + incl - size;
    for (uint32_t j = 0; j < here; ++j)
      wave_emit(out + uint32_t(__shfl(mine, int(j))), in + uint32_t(__shfl(prev, int(j))),
                uint32_t(__shfl(lit, int(j))), uint32_t(__shfl(len, int(j))), uint32_t(__shfl(off, int(j))), lane);
    o += uint32_t(__shfl(incl, kWave - 1));
    prev_end = uint32_t(__shfl(end, int(here - 1)));
  }
  if (g + 1 == ws.chunk_base[b + 1]) {  // the block's last chunk also writes the last literal run
    const uint32_t anchor = ws.fin_anchor[b];
    wave_emit(out + ws.fin_off[b], in + anchor, n - anchor, 0, 0, lane);
  }
}

int launched() { return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR; }

uint64_t align16(uint64_t v) { return (v + 15) & ~UINT64_C(15); }

}  // namespace

rpp_lz4::EncodeWs rpp_lz4::carve_workspace(void* d_workspace, uint64_t total_bytes, uint32_t nblocks) {
  const uint64_t mc = max_chunks_of(total_bytes, nblocks);
  uint8_t* p = static_cast<uint8_t*>(d_workspace);
  auto take = [&p](uint64_t bytes) {
    uint32_t* r = reinterpret_cast<uint32_t*>(p);
    p += align16(bytes);
    return r;
  };
  EncodeWs ws{};
  ws.chunk_base = take(4ull * (nblocks + 1));
  ws.ok = take(16);
  ws.fin_anchor = take(4ull * nblocks);
  ws.fin_off = take(4ull * nblocks);
  ws.cnt = take(4 * mc);
  ws.first_pos = take(4 * mc);
  ws.last_end = take(4 * mc);
  ws.body = take(4 * mc);
  ws.carry = take(4 * mc);
  ws.out_off = take(4 * mc);
  ws.seqs = reinterpret_cast<uint2*>(p);
  ws.max_chunks = uint32_t(mc);
  return ws;
}

void rpp_lz4::launch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                            uint32_t nblocks, const EncodeWs& ws, uint64_t* d_out_bytes, uint32_t* d_flags,
                            int32_t* d_status, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_lz4_prep_kernel, dim3(1), dim3(kWave), 0, s, d_in_bytes, nblocks, ws, d_out_bytes, d_flags,
                     d_status);
  hipLaunchKernelGGL(rpp_lz4_search_kernel, dim3(ws.max_chunks), dim3(kWave), 0, s, d_in, d_in_offsets, d_in_bytes,
                     nblocks, ws);
}

void rpp_lz4::launch_search(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                            uint32_t nblocks, const EncodeWs& ws, uint64_t* d_out_bytes, uint32_t* d_flags,
                            int32_t* d_status, uint32_t search, void* stream) {
  if (search == 0)
    return launch_search(d_in, d_in_offsets, d_in_bytes, nblocks, ws, d_out_bytes, d_flags, d_status, stream);
  hipLaunchKernelGGL(rpp_lz4_prep_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), d_in_bytes,
                     nblocks, ws, d_out_bytes, d_flags, d_status);
  launch_deep_search(d_in, d_in_offsets, d_in_bytes, nblocks, ws, search, stream);
}

extern "C" int rpp_lz4_decode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                    uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                    const uint64_t* d_out_bytes, int32_t* d_status, void* stream) {
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_out || !d_out_offsets || !d_out_bytes || !d_status)
    return RPP_INVALID_ARGUMENT;
  hipLaunchKernelGGL(rpp_lz4_decode_kernel, dim3((nblocks + kDecodeWaves - 1) / kDecodeWaves),
                     dim3(kWave * kDecodeWaves), 0, static_cast<hipStream_t>(stream), d_in, d_in_offsets, d_in_bytes,
                     nblocks, d_out, d_out_offsets, d_out_bytes, d_status);
  return launched();
}

extern "C" uint64_t rpp_lz4_encode_workspace_bytes(uint64_t total_bytes, uint32_t nblocks) {
  const uint64_t mc = max_chunks_of(total_bytes, nblocks);
  return align16(4ull * (nblocks + 1)) + 16 + 2 * align16(4ull * nblocks) + 6 * align16(4 * mc) +
         mc * kSeqsPerChunk * sizeof(uint2);
}

extern "C" int rpp_lz4_encode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                    uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                    uint64_t* d_out_bytes, uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                    void* d_workspace, uint64_t workspace_bytes, void* stream) {
  return rpp_lz4_encode_batch_search(d_in, d_in_offsets, d_in_bytes, nblocks, 0, d_out, d_out_offsets, d_out_bytes,
                                     d_flags, d_status, total_bytes, d_workspace, workspace_bytes, stream);
}

static_assert(RPP_SEARCH_LAZY == kSearchLazy, "the search word");

extern "C" int rpp_lz4_encode_batch_search(const uint8_t* d_in, const uint64_t* d_in_offsets,
                                           const uint64_t* d_in_bytes, uint32_t nblocks, uint32_t search,
                                           uint8_t* d_out, const uint64_t* d_out_offsets, uint64_t* d_out_bytes,
                                           uint32_t* d_flags, int32_t* d_status, uint64_t total_bytes,
                                           void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (!search_valid(search)) return RPP_INVALID_ARGUMENT;
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_out || !d_out_offsets || !d_out_bytes || !d_flags || !d_status ||
      !d_workspace || ((uintptr_t)d_workspace & 15))
    return RPP_INVALID_ARGUMENT;
  const uint64_t mc = max_chunks_of(total_bytes, nblocks);
  if (mc >= 0x7fffffffu) return RPP_INVALID_ARGUMENT;
  if (workspace_bytes < rpp_lz4_encode_workspace_bytes(total_bytes, nblocks)) return RPP_OUTPUT_TOO_SMALL;
  const EncodeWs ws = carve_workspace(d_workspace, total_bytes, nblocks);
  launch_search(d_in, d_in_offsets, d_in_bytes, nblocks, ws, d_out_bytes, d_flags, d_status, search, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_lz4_place_kernel, dim3(nblocks), dim3(kWave), 0, s, d_in_bytes, nblocks, ws, d_out,
                     d_out_offsets, d_out_bytes, d_flags, d_status);
  hipLaunchKernelGGL(rpp_lz4_emit_kernel, dim3(uint32_t(mc)), dim3(kWave), 0, s, d_in, d_in_offsets, d_in_bytes,
                     nblocks, ws, d_out, d_out_offsets);
  return launched();
}
