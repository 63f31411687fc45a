// ricepp_encode.hip -- MI355X (gfx950) ricepp encode kernels and the encode
// entry points of the C ABI declared in include/ricepp_amd.h.
//
// Bitstream format: ricepp (mhx/dwarfs ricepp/, restated in SURVEY.md
// Appendix A).  One wavefront owns one independent stream (a DwarFS block);
// streams shard across the grid with no inter-wave communication.
//
// Encode (per wave, loop over groups of sub-blocks):
//   * a sub-block of `bs` samples is owned by an aligned group of G lanes
//     (G = next pow2 of ceil(bs/8)), each lane holding 8 samples;
//   * zig-zag deltas in registers, per-sub-block cost(fs) by group
//     reductions, exact replay of compute_best_split's hill climb
//     (ricepp/include/ricepp/detail/encode.h:43-90);
//   * code lengths -> one wave-wide prefix scan -> absolute bit positions;
//   * codes OR-ed into an LDS window (ds_or_b32), complete 16-byte chunks
//     streamed to HBM with coalesced dwordx4 stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ricepp_amd.h"
#include "ricepp_internal.h"
#include "ricepp_stats.h"
#include "ricepp_wave.h"

#ifdef RPP_STATS
__device__ unsigned long long g_enc_stats[16];
#endif

namespace {

struct EncParams {
  const uint16_t* in;
  const uint64_t* in_off;
  const uint64_t* n_samples;
  uint8_t* out;
  const uint64_t* out_off;
  uint64_t* out_bytes;
  int32_t* status;
  uint32_t nblocks;
  uint32_t bs, cs, be, ulsb;
  // segment mode (long streams, rpp_encode_batch_ws): work unit u = segment
  // u - seg_base[b] of stream b = seg_map[u]; null seg_map: unit = stream
  const uint32_t* seg_map;
  const uint64_t* seg_base;  // [nblocks + 1]: units before stream b; [nblocks] = total
  uint64_t* seg_bits;        // [units] bits a segment wrote (multi-segment streams)
  uint8_t* scratch;          // segments >= 1 of a stream: slot u - b - 1
  uint64_t slot_bytes;
  // units the workspace holds: a batch with more (its samples exceed the
  // caller's total_samples) is encoded one wave per stream, nothing split
  uint64_t max_units;
  uint32_t seg_chunks;  // chunks per unit (enc_seg_chunks)
};
// segment mode and the batch fits the workspace
__device__ __forceinline__ bool enc_split_ok(const EncParams& p) {
  return p.seg_map && p.seg_base[p.nblocks] <= p.max_units;
}

// Segment mode: a stream of more than seg_chunks chunks is encoded by
// several waves, one per run of seg_chunks chunks.  Every sub-block's codes
// depend only on its samples and the sample before it (encode.h:92-157), so a
// segment starts from the real preceding sample, at bit 0 of its own scratch
// slot (segment 0: after the initial values, in the stream's output), and
// rpp_enc_concat_kernel then places each segment at its bit offset.
// seg_chunks is kEncSegChunks when the batch fills the GPU with units of that
// size, smaller (down to kEncSegChunksMin, so that a unit that is not its
// stream's last holds at least 64 bits) for batches of few blocks, whose
// latency is one wave's pass over a whole block otherwise (enc_seg_chunks)
constexpr uint32_t kEncSegChunks = 256;
constexpr uint32_t kEncSegChunksMin = 16;
constexpr uint64_t kEncTargetUnits = 2048;
// wave priority in the pipelined encode: plans (deltas, split walk,
// positions) at priority 1, the LDS emission at 0 (the reverse and no
// priority measured slower: DESIGN.md §4 "Wave priority")

// Compile-time shape of an encode launch: SPL samples per lane (8 or 16), a
// ricepp sub-block owned by an aligned group of G lanes (G = next pow2 of
// ceil(bs / SPL)), CS component streams.  64 / G sub-blocks per iteration.

// Sum over the aligned group of G lanes containing this lane, broadcast to
// every lane of the group (butterfly; all lanes active).
template <uint32_t G>
__device__ __forceinline__ uint32_t gsum(uint32_t v) {
  if constexpr (G >= 2) v += dpp<kDppQuadXor1>(v);
  if constexpr (G >= 4) v += dpp<kDppQuadXor2>(v);
  if constexpr (G >= 8) v += dpp<kDppRowHalfMirror>(v);
  if constexpr (G >= 16) v += dpp<kDppRowMirror>(v);
  if constexpr (G >= 32) {
    auto t = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = t[0] + t[1];
  }
  if constexpr (G >= 64) {
    auto t = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    v = t[0] + t[1];
  }
  return v;
}

// Per-lane sub-block geometry of one encode iteration.
struct EncGeom {
  uint32_t n;        // samples in this lane's sub-block (0: no sub-block)
  uint32_t cnt;      // samples owned by this lane (<= SPL)
  uint32_t m_first;  // stream index of the lane's first sample
  uint32_t comp;     // component stream
};

template <uint32_t SPL, uint32_t CS>
__device__ __forceinline__ EncGeom enc_geom(uint32_t s, uint32_t j, uint32_t nsb, uint32_t N, uint32_t bs) {
  EncGeom g;
  // codec.h:88-97: chunks of cs*bs samples; component i takes i, i+cs, ...
  const uint32_t chunk = s / CS;
  g.comp = s % CS;
  const uint32_t cbase = chunk * CS * bs;
  g.n = 0;
  if (s < nsb) {
    const uint32_t rem = (N - cbase) / CS;
    g.n = rem < bs ? rem : bs;
  }
  const uint32_t k0 = SPL * j;
  g.cnt = k0 < g.n ? min(g.n - k0, SPL) : 0u;
  g.m_first = cbase + g.comp + CS * k0;
  return g;
}

// The lane's stored samples as SPL / 2 packed pairs (sample 2k in the low
// half of w[k]) plus the previous same-component stored sample.
template <uint32_t SPL>
struct EncRaw {
  uint32_t w[SPL / 2];
  uint32_t prev;
};

// Full iterations (every lane owns 0 or SPL samples): 16-byte loads.
template <uint32_t SPL, uint32_t CS>
__device__ __forceinline__ EncRaw<SPL> enc_load_vec(const uint16_t* in, const EncGeom& g, bool load_prev) {
  EncRaw<SPL> r;
  // codec.h:72-73: a component's first sample is its own reference (last = read(in[i]))
  if (load_prev) {
    const uint32_t pi = g.cnt ? (g.m_first >= CS ? g.m_first - CS : g.m_first) : 0u;
    r.prev = in[pi];
  } else {
    r.prev = 0;
  }
  const uint4* q = reinterpret_cast<const uint4*>(g.cnt ? in + (g.m_first - g.comp) : in);
  if constexpr (CS == 1) {
#pragma unroll
    for (uint32_t i = 0; i < SPL / 8; ++i) {
      const uint4 v = q[i];
      r.w[4 * i] = v.x; r.w[4 * i + 1] = v.y; r.w[4 * i + 2] = v.z; r.w[4 * i + 3] = v.w;
    }
  } else {
    // interleaved (c0, c1) pairs: keep this lane's component
    const uint32_t sel = g.comp ? 0x07060302u : 0x05040100u;
#pragma unroll
    for (uint32_t i = 0; i < SPL / 4; ++i) {
      const uint4 v = q[i];
      r.w[2 * i] = __builtin_amdgcn_perm(v.y, v.x, sel);
      r.w[2 * i + 1] = __builtin_amdgcn_perm(v.w, v.z, sel);
    }
  }
  return r;
}

// Ragged tail / unaligned streams: per-sample loads.
template <uint32_t SPL, uint32_t CS>
__device__ __forceinline__ EncRaw<SPL> enc_load_scalar(const uint16_t* in, const EncGeom& g) {
  EncRaw<SPL> r;
  const uint32_t pi = g.m_first >= CS ? g.m_first - CS : g.m_first;
  r.prev = g.cnt ? (uint32_t)in[pi] : 0u;
#pragma unroll
  for (uint32_t k = 0; k < SPL / 2; ++k) {
    const uint32_t lo = 2 * k < g.cnt ? (uint32_t)in[g.m_first + CS * 2 * k] : 0u;
    const uint32_t hi = 2 * k + 1 < g.cnt ? (uint32_t)in[g.m_first + CS * (2 * k + 1)] : 0u;
    r.w[k] = lo | (hi << 16);
  }
  return r;
}

// ORs the (<= 16 bit) code `v` into the window at bit `rel` (two ds_or_b32;
// the second is 0 when the code does not straddle a word).
__device__ __forceinline__ void emit_bits(uint32_t* win, uint32_t rel, uint32_t v) {
  const uint32_t w = rel >> 5, sh = rel & 31u;
  atomicOr(&win[w], v << sh);
  atomicOr(&win[w + 1], (v >> 1) >> (31u - sh));
}

// The same for codes of <= 32 bits.  32-bit shifts only: a 64-bit shift
// (v_lshlrev_b64) whose amount the register allocator happens to place in the
// last VGPR of the kernel's allocation reads a wrong amount on gfx950 while
// other waves share the SIMD -- the round-5 bs 128 cs 2 fault (DESIGN.md §4
// "64-bit shifts and the last VGPR"; tools/isa_audit.py guards the build).
__device__ __forceinline__ void emit_bits64(uint32_t* win, uint32_t rel, uint32_t v) {
  const uint32_t sh = rel & 31u;
  uint32_t* w = win + (rel >> 5);
  atomicOr(w, v << sh);
  atomicOr(w + 1, (v >> 1) >> (31u - sh));
}

constexpr uint32_t kEncWin = 1024;      // LDS output window (words, 4 KiB)
constexpr uint32_t kEncFlushWords = 256;  // stream out once >= 1 KiB of whole 64-byte lines is ready

struct EncState {
  uint32_t* win;
  uint32_t* out32;
  uint32_t win_w0;  // global word index held in win[0] (multiple of 16)
  uint32_t base;       // absolute bit position after the emitted codes
  uint32_t plan_base;  // absolute bit position after the planned codes
  uint32_t carry;      // pixel value of the sample before this iteration (DPP-prev mode)
};

// sum over the lane's samples of d >> f (the lane's unary bits at fs = f)
template <uint32_t SPL>
__device__ __forceinline__ uint32_t enc_shr_sum(const us2* d, uint32_t f) {
  const us2 fv = (us2)(unsigned short)f, one = {1, 1};
  uint32_t acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < SPL / 2; ++k) acc = __builtin_amdgcn_udot2(d[k] >> fv, one, acc, false);
  return acc;
}

// One group of 64/G sub-blocks is encoded in three steps, so that the full
// iterations can be software-pipelined (the plan of group i+1 is computed
// while group i is emitted):
//   enc_plan_a: zig-zag deltas, sums, compute_best_split start and first pair
//   enc_plan_b: the split walk, mode, bit positions by one wave scan
//   enc_emit:   header and codes OR-ed into the LDS window
// dpp_prev: every lane full and the previous sample of a lane's first sample
// is the previous lane's last one (CS == 1, bs == G * SPL): no prev loads.
template <uint32_t SPL>
struct EncPlan {
  us2 d[SPL / 2];       // zig-zag deltas
  uint32_t w[SPL / 2];  // stored samples (raw sub-blocks)
  uint32_t n, cnt, sum;
  uint32_t bits, lq;    // best cost so far, this lane's unary bits at that fs
  int cand, dir;
  bool walking;
  uint32_t mode, fs;    // 0 = all-zero, 1 = Rice, 2 = raw
  uint32_t pos;         // absolute bit position of this lane's first bit
  uint32_t end;         // absolute bit position after the group
};

template <uint32_t SPL, uint32_t G, uint32_t CS, bool SH>
__device__ __forceinline__ void enc_plan_a(EncPlan<SPL>& P, EncState& st, const EncRaw<SPL>& r, const EncGeom& geo,
                                           uint32_t selbe, uint32_t be, uint32_t ulsb, bool mask_tail,
                                           bool dpp_prev) {
  constexpr uint32_t NW = SPL / 2;
  const uint32_t n = geo.n, cnt = geo.cnt;
  P.n = n;
  P.cnt = cnt;
  const bool sb_valid = n != 0;
  // ---- pixel values (ricepp_cpuspecific_traits.h:63-67) and zig-zag deltas
  //      (encode.h:116-123), two samples per instruction ----
  us2 v[NW];
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) {
    P.w[k] = r.w[k];
    v[k] = as_us2(__builtin_amdgcn_perm(r.w[k], r.w[k], selbe));
    if constexpr (SH) v[k] = v[k] >> (us2)(unsigned short)ulsb;
  }
  uint32_t pv;
  if (dpp_prev) {
    const uint32_t lastv = as_u32(v[NW - 1]) >> 16;
    pv = dpp_keep<kDppWaveShr1>(st.carry, lastv);  // lane 0: the carried sample
    st.carry = readlane(lastv, kWave - 1);
  } else {
    pv = px_read(r.prev, be, ulsb);
  }
  uint32_t prevw = pv << 16;
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) {
    const us2 pp = as_us2(__builtin_amdgcn_alignbit(as_u32(v[k]), prevw, 16));
    prevw = as_u32(v[k]);
    const us2 diff = v[k] - pp;
    P.d[k] = (diff << (us2)1) ^ as_us2(__builtin_bit_cast(uint32_t, (__builtin_bit_cast(ss2, diff) >> (ss2)15)));
  }
  if (mask_tail) {
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) {
      const uint32_t keep = (2u * k < cnt ? 0xFFFFu : 0u) | (2u * k + 1 < cnt ? 0xFFFF0000u : 0u);
      P.d[k] = as_us2(as_u32(P.d[k]) & keep);
    }
  }
  const us2 one = {1, 1};
  uint32_t lsum = 0;
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) lsum = __builtin_amdgcn_udot2(P.d[k], one, lsum, false);
  const uint32_t sum = gsum<G>(lsum);
  P.sum = sum;

  // ---- compute_best_split replay (encode.h:43-90), first pair ----
  // start = max(0, bit_width(sum / n) - 2) without a division:
  // bit_width(floor(s/n)) = t + (s >= n << t), t = floor(log2 s) - floor(log2 n)
  uint32_t bwq = 0;
  if (n != 0 && sum >= n) {
    const uint32_t t = (uint32_t)__clz(n) - (uint32_t)__clz(sum);
    bwq = t + ((n << t) <= sum ? 1u : 0u);
  }
  const uint32_t start = bwq >= 2 ? bwq - 2 : 0u;
  // (the lane's share of the unary bits of the current candidate is kept:
  // the chosen fs needs it again for the bit positions)
  const uint32_t lq0 = enc_shr_sum<SPL>(P.d, start), lq1 = enc_shr_sum<SPL>(P.d, start + 1);
  const uint32_t bits0 = n * (start + 1) + gsum<G>(lq0);
  const uint32_t bits1 = n * (start + 2) + gsum<G>(lq1);
  if (bits1 <= bits0) {
    P.cand = (int)start + 1; P.bits = bits1; P.dir = 1; P.lq = lq1;
  } else {
    P.cand = (int)start; P.bits = bits0; P.dir = -1; P.lq = lq0;
  }
  P.walking = sb_valid && sum != 0 && bits0 != bits1;
}

template <uint32_t SPL, uint32_t G>
__device__ __forceinline__ void enc_plan_b(EncPlan<SPL>& P, EncState& st, uint32_t j) {
  const uint32_t n = P.n, cnt = P.cnt;
  const bool sb_valid = n != 0;
  // ---- compute_best_split replay: the walk.  Almost every sub-block takes
  //      exactly one more candidate (that does not improve), so the first
  //      step runs unconditionally, without a vote and a branch ----
  auto walk_step = [&](bool act) {
    const uint32_t f = act ? (uint32_t)(P.cand + P.dir) : 0u;
    const uint32_t lt = enc_shr_sum<SPL>(P.d, f);
    const uint32_t t = n * (f + 1) + gsum<G>(lt);
    if (act && t <= P.bits) {
      P.bits = t;
      P.lq = lt;
      P.cand += P.dir;
    } else {
      P.walking = false;
    }
  };
  walk_step(P.walking && P.cand > 0 && P.cand < 14);
  for (;;) {
    const bool act = P.walking && P.cand > 0 && P.cand < 14;
    if (!__any(act)) break;
    walk_step(act);
  }
  // encode.h:127-156: 0 = all-zero, 1 = Rice, 2 = raw
  P.mode = 0;
  P.fs = 0;
  if (sb_valid && P.sum != 0) {
    P.fs = (uint32_t)P.cand;
    P.mode = (P.fs < 14 && P.bits < 16 * n) ? 1u : 2u;
  }
  // ---- bit positions: one wave-wide scan ----
  uint32_t lbits = (sb_valid && j == 0) ? 4u : 0u;
  if (P.mode == 1) lbits += P.lq + cnt * (P.fs + 1);
  else if (P.mode == 2) lbits += 16 * cnt;
  const uint32_t incl = wave_incl_sum(lbits);
  P.pos = st.plan_base + incl - lbits;
  st.plan_base += readlane(incl, kWave - 1);
  P.end = st.plan_base;
}

template <uint32_t SPL>
__device__ __forceinline__ void enc_emit(const EncPlan<SPL>& P, EncState& st, uint32_t j, bool mask_tail) {
  const uint32_t cnt = P.cnt, mode = P.mode, fs = P.fs;
  uint32_t pos = P.pos - 32 * st.win_w0;  // window-relative
  if (P.n != 0 && j == 0) {
    emit_bits(st.win, pos, mode == 0 ? 0u : (mode == 1 ? fs + 1 : 15u));
    pos += 4;
  }
  if (mode == 1 && !mask_tail) {
    // every lane owns SPL samples: two codes per packed step.  The '1' of
    // code i sits at e_i = e_(i-1) + k + q_i; the code value (1 | r << 1,
    // <= 15 bits) is OR-ed in by one 64-bit shift and two ds_or_b32.
    const uint32_t k = fs + 1;
    const uint32_t m2 = ((2u << fs) - 1u) * 0x10001u;
    uint32_t e = pos - k;
    us2 qv[SPL / 2];
    us2 qmax = {0, 0};
#pragma unroll
    for (uint32_t h = 0; h < SPL / 2; ++h) {
      qv[h] = P.d[h] >> (us2)(unsigned short)fs;
      qmax = __builtin_elementwise_max(qmax, qv[h]);
    }
    // the pair (2h, 2h+1) spans k + q_(2h+1) + k bits from code 2h's '1':
    // when that fits 32 bits for every pair of the wave (fs <= 13 and unary
    // runs short: Poisson data), one 64-bit shift and two ds_or_b32 per pair
    if (!__any(2u * k + (as_u32(qmax) >> 16) > 32u)) {
#pragma unroll
      for (uint32_t h = 0; h < SPL / 2; ++h) {
        const uint32_t qq = as_u32(qv[h]);
        const uint32_t cc = (as_u32(P.d[h] << (us2)1) & m2) | 0x10001u;
        e += k + (qq & 0xFFFFu);
        const uint32_t d = k + (qq >> 16);
        emit_bits64(st.win, e, (cc & 0xFFFFu) | ((cc >> 16) << d));
        e += d;
      }
    } else {
#pragma unroll
      for (uint32_t h = 0; h < SPL / 2; ++h) {
        const uint32_t qq = as_u32(qv[h]);
        const uint32_t cc = (as_u32(P.d[h] << (us2)1) & m2) | 0x10001u;
        e += k + (qq & 0xFFFFu);
        emit_bits64(st.win, e, cc & 0xFFFFu);
        e += k + (qq >> 16);
        emit_bits64(st.win, e, cc >> 16);
      }
    }
  } else if (mode == 1) {
    const uint32_t lowmask = (1u << fs) - 1u;
#pragma unroll
    for (uint32_t i = 0; i < SPL; ++i) {
      if (i < cnt) {
        const uint32_t di = (i & 1) ? (as_u32(P.d[i >> 1]) >> 16) : (as_u32(P.d[i >> 1]) & 0xFFFFu);
        pos += di >> fs;  // unary zeros are implicit (the window is zeroed)
        emit_bits(st.win, pos, 1u | ((di & lowmask) << 1));
        pos += fs + 1;
      }
    }
  } else if (mode == 2) {
#pragma unroll
    for (uint32_t i = 0; i < SPL; ++i) {
      if (i < cnt) {
        const uint32_t ri = (i & 1) ? (P.w[i >> 1] >> 16) : (P.w[i >> 1] & 0xFFFFu);
        emit_bits(st.win, pos, ri);  // raw stored value (encode.h:148-151)
        pos += 16;
      }
    }
  }
  st.base = P.end;
}

// The three steps back to back (ragged tails, unpipelined groups).
template <uint32_t SPL, uint32_t G, uint32_t CS, bool SH>
__device__ __forceinline__ void enc_iteration(EncState& st, const EncRaw<SPL>& r, const EncGeom& geo, uint32_t j,
                                              uint32_t selbe, uint32_t be, uint32_t ulsb, bool mask_tail,
                                              bool dpp_prev) {
  EncPlan<SPL> P;
  enc_plan_a<SPL, G, CS, SH>(P, st, r, geo, selbe, be, ulsb, mask_tail, dpp_prev);
  enc_plan_b<SPL, G>(P, st, j);
  enc_emit<SPL>(P, st, j, mask_tail);
}

// Streams whole 64-byte lines out once >= kEncFlushWords are complete.
__device__ __forceinline__ void enc_flush(EncState& st, bool final_flush) {
  const uint32_t lane = lane_id();
  wave_lds_fence();
  const uint32_t full_end = st.base >> 5;  // words before it are complete
  const uint32_t F = full_end & ~15u;
  if (F >= st.win_w0 + kEncFlushWords || (final_flush && F > st.win_w0)) {
    const uint32_t nch = (F - st.win_w0) >> 2;
    for (uint32_t c = lane; c < nch; c += kWave) {
      const uint4 v = *reinterpret_cast<const uint4*>(&st.win[4 * c]);
      *reinterpret_cast<uint4*>(&st.out32[st.win_w0 + 4 * c]) = v;
    }
    const uint32_t used = full_end - st.win_w0 + 1;
    const uint32_t tail0 = F - st.win_w0;
    const uint32_t keep = lane < 16 ? st.win[tail0 + lane] : 0u;
    wave_lds_fence();
    for (uint32_t i = lane; i < used; i += kWave) st.win[i] = 0;
    wave_lds_fence();
    if (lane < 16) st.win[lane] = keep;
    wave_lds_fence();
    st.win_w0 = F;
  }
}

// SH: unused_lsb_count != 0 (the pixel read shifts)
template <uint32_t SPL, uint32_t G, uint32_t CS, bool SH>
__global__ __launch_bounds__(kWave) void rpp_encode_kernel(EncParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t win[kEncWin];
  constexpr uint32_t spw = kWave / G;  // sub-blocks per iteration
  uint32_t b = blockIdx.x, seg = 0;
  const bool split = enc_split_ok(p);
  if (split) {
    if (blockIdx.x >= p.seg_base[p.nblocks]) return;
    b = p.seg_map[blockIdx.x];
    seg = blockIdx.x - (uint32_t)p.seg_base[b];
  } else if (b >= p.nblocks) {
    return;
  }
  const uint32_t lane = lane_id();
  const uint32_t bs = p.bs, be = p.be, ulsb = p.ulsb;
  const uint32_t selbe = be ? 0x02030001u : 0x03020100u;
  const uint64_t n64 = p.n_samples[b];
  const uint64_t ooff = p.out_off[b];
  if (n64 % CS != 0 || n64 >= RPP_MAX_STREAM_SAMPLES || (ooff & 15u)) {
    if (lane == 0 && seg == 0) {
      p.status[b] = RPP_INVALID_ARGUMENT;
      p.out_bytes[b] = 0;
    }
    return;
  }
  const uint32_t N = (uint32_t)n64;
  const uint16_t* in = p.in + p.in_off[b];
  const uint32_t chunk_len = CS * bs;
  const uint32_t nchunks = (N + chunk_len - 1) / chunk_len;
  const uint32_t segc = p.seg_chunks;
  const bool multi = split && nchunks > segc;
  // one wave for a whole stream keeps 32-bit bit positions: longer streams
  // must be split (rpp_encode_batch_ws)
  if (!multi && n64 >= rpp_internal::kSegMaxSamples) {
    if (lane == 0 && seg == 0) {
      p.status[b] = RPP_INVALID_ARGUMENT;
      p.out_bytes[b] = 0;
    }
    return;
  }
  // this unit's chunks [c_lo, c_hi)
  const uint32_t c_lo = multi ? seg * segc : 0u;
  const uint32_t c_hi = multi ? min(nchunks, c_lo + segc) : nchunks;
  uint8_t* out8 = seg == 0 ? p.out + ooff : p.scratch + (size_t)(blockIdx.x - b - 1) * p.slot_bytes;
#ifdef RPP_STATS
  uint32_t stat_acc[16] = {0};
  unsigned long long tprev_;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev_)::"memory");
#endif

  for (uint32_t i = lane; i < kEncWin; i += kWave) win[i] = 0;
  __syncthreads();

  const uint32_t bit0 = seg == 0 ? 16 * CS : 0u;
  EncState st{win, reinterpret_cast<uint32_t*>(out8), 0u, bit0, bit0, 0u};
  // codec.h:69-74,81-86: 16-bit initial value read(in[i]) per component.
  if (seg == 0 && lane < CS) emit_bits(win, 16 * lane, N ? px_read(in[lane], be, ulsb) : 0u);
  // DPP-prev mode: the reference of the unit's first sample (the stream's
  // first sample is its own reference)
  st.carry = N ? px_read(in[c_lo ? c_lo * chunk_len - 1 : 0], be, ulsb) : 0u;

  const uint32_t nsb = c_hi * CS;     // sub-blocks [s_lo, nsb) are this unit's
  const uint32_t s_lo = c_lo * CS;
  const uint32_t g = lane / G, j = lane % G;
  // full iterations: every sub-block complete, lanes own 0 or SPL samples
  const bool vec_ok = bs % SPL == 0 && ((uintptr_t)in & 15u) == 0;
  const uint32_t nsb_full = vec_ok ? min(N / chunk_len, c_hi) * CS : 0u;
  const uint32_t nfull = nsb_full > s_lo ? (nsb_full - s_lo) / spw : 0u;
  const bool empty_lanes = G * SPL != bs;
  const bool dpp_prev = CS == 1 && !empty_lanes;

  // ---- full iterations, software-pipelined: group it+1 is planned
  //      (deltas, split, positions) around the emission of group it, so the
  //      two dependency chains overlap.  Two sample buffers: the one just
  //      planned from is reloaded at once with the group after next, about
  //      two steps before its use; unrolled by two so that plans and loaded
  //      samples stay in place (no register copies) ----
  uint32_t it = 0;
  if (nfull) {
    EncGeom g0 = enc_geom<SPL, CS>(s_lo + g, j, nsb, N, bs);
    EncRaw<SPL> r0 = enc_load_vec<SPL, CS>(in, g0, !dpp_prev);
    EncGeom g1 = enc_geom<SPL, CS>(s_lo + spw + g, j, nsb, N, bs);
    EncRaw<SPL> r1 = enc_load_vec<SPL, CS>(in, g1, !dpp_prev);
    EncPlan<SPL> P, Q;
    enc_plan_a<SPL, G, CS, SH>(P, st, r0, g0, selbe, be, ulsb, empty_lanes, dpp_prev);
    // (loads are unconditional: past the last group the geometry is empty
    // and the load reads the stream start; a conditional load would make
    // every later wait cover it)
    g0 = enc_geom<SPL, CS>(s_lo + 2 * spw + g, j, nsb, N, bs);
    r0 = enc_load_vec<SPL, CS>(in, g0, !dpp_prev);
    enc_plan_b<SPL, G>(P, st, j);
    // emits group `it` (plan E) while planning group it+1 (into F, from rn,
    // which then takes group it+3)
    auto step = [&](EncPlan<SPL>& E, EncPlan<SPL>& F, EncRaw<SPL>& rn, EncGeom& gn) {
      RPP_STAT(0, 1);
      RPP_TSTAMP(1);
      __builtin_amdgcn_s_setprio(1);
      enc_plan_a<SPL, G, CS, SH>(F, st, rn, gn, selbe, be, ulsb, empty_lanes, dpp_prev);
      gn = enc_geom<SPL, CS>(s_lo + (it + 3) * spw + g, j, nsb, N, bs);
      rn = enc_load_vec<SPL, CS>(in, gn, !dpp_prev);
      RPP_TSTAMP(2);
      __builtin_amdgcn_s_setprio(0);
      enc_emit<SPL>(E, st, j, empty_lanes);
      __builtin_amdgcn_s_setprio(1);
      RPP_TSTAMP(3);
      enc_plan_b<SPL, G>(F, st, j);
      __builtin_amdgcn_s_setprio(0);
      RPP_TSTAMP(4);
      enc_flush(st, false);
      RPP_TSTAMP(5);
      ++it;
    };
    while (it + 1 < nfull) {
      step(P, Q, r1, g1);  // P = group it, r1 = group it+1 -> Q
      if (it + 1 >= nfull) break;
      step(Q, P, r0, g0);  // Q = group it, r0 = group it+1 -> P
    }
    // the last group: in P after an even number of steps, else in Q
    enc_emit<SPL>((it & 1) ? Q : P, st, j, empty_lanes);
    enc_flush(st, false);
    ++it;
  }
  // ---- ragged tail / unaligned streams: per-sample loads ----
  for (uint32_t s0 = s_lo + it * spw; s0 < nsb; s0 += spw) {
    const EncGeom geo = enc_geom<SPL, CS>(s0 + g, j, nsb, N, bs);
    const EncRaw<SPL> r = enc_load_scalar<SPL, CS>(in, geo);
    enc_iteration<SPL, G, CS, SH>(st, r, geo, j, selbe, be, ulsb, true, false);
    enc_flush(st, false);
  }
  enc_flush(st, true);

  // ---- final words and the ceil(bits/8) tail bytes
  //      (bitstream_writer.h:110-120,139-145) ----
  const uint32_t total_bytes = (st.base + 7) >> 3;
  const uint32_t full_end = st.base >> 5;
  if (multi && seg != 0) {
    // a segment slot: whole words (the last one zero-padded) for the concat
    for (uint32_t w = st.win_w0 + lane; w <= full_end; w += kWave) st.out32[w] = win[w - st.win_w0];
  } else {
    for (uint32_t w = st.win_w0 + lane; w < full_end; w += kWave) st.out32[w] = win[w - st.win_w0];
    const uint32_t tail_bytes = total_bytes - 4 * full_end;
    if (lane < tail_bytes) out8[4 * full_end + lane] = (uint8_t)(win[full_end - st.win_w0] >> (8 * lane));
  }
  if (lane == 0) {
    if (multi) {
      p.seg_bits[blockIdx.x] = st.base;  // (the concat kernel writes size and status)
    } else {
      p.out_bytes[b] = total_bytes;
      p.status[b] = RPP_OK;
    }
  }
#ifdef RPP_STATS
  if (lane == 0)
    for (int i = 0; i < 16; ++i) atomicAdd(&g_enc_stats[i], (unsigned long long)stat_acc[i]);
#endif
}

// Units of each stream (nseg: one per seg_chunks chunks for a stream of
// more than seg_chunks chunks, else 1); entry nblocks is 0 so the exclusive
// scan ends in the total.
__global__ void rpp_enc_units_kernel(const uint64_t* n_samples, uint32_t nblocks, uint32_t chunk_len,
                                     uint32_t seg_chunks, uint64_t* units) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nblocks) return;
  uint64_t u = 0;
  if (i < nblocks) {
    const uint64_t n = n_samples[i];
    const uint64_t nch = (n + chunk_len - 1) / chunk_len;
    u = nch > seg_chunks && n < RPP_MAX_STREAM_SAMPLES ? (nch + seg_chunks - 1) / seg_chunks : 1;
  }
  units[i] = u;
}

__global__ void rpp_enc_unit_map_kernel(const uint64_t* seg_base, uint32_t nblocks, uint64_t max_units,
                                        uint32_t* seg_map) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nblocks || seg_base[nblocks] > max_units) return;  // (over the workspace: nothing is split)
  for (uint64_t u = seg_base[i]; u < seg_base[i + 1]; ++u) seg_map[u] = i;
}

// Places segment k >= 1 of a multi-segment stream at its bit offset o_k in the
// stream's output (seg_off = exclusive scan of seg_bits over all units).  An
// output word belongs to the segment holding its first bit and takes the
// following segment's first bits above that segment's end; the word holding
// o_1 (partly written by segment 0 in place) is merged by segment 1.  The
// last word is written byte by byte up to ceil(bits / 8)
// (bitstream_writer.h:139-145); the last segment writes size and status.
__global__ __launch_bounds__(256) void rpp_enc_concat_kernel(EncParams p, const uint64_t* seg_off) {
  const uint32_t u = blockIdx.x;
  if (!enc_split_ok(p) || u >= p.seg_base[p.nblocks]) return;
  const uint32_t b = p.seg_map[u];
  const uint32_t first = (uint32_t)p.seg_base[b], nseg = (uint32_t)(p.seg_base[b + 1] - first);
  const uint32_t k = u - first;
  if (nseg < 2 || k == 0) return;
  // (bit offsets in the stream are 64-bit: streams go up to 2^30 samples;
  // word indices fit 32 bits)
  const uint64_t base = seg_off[first];
  const uint64_t o_k = seg_off[u] - base;
  const uint32_t L_k = (uint32_t)p.seg_bits[u];
  const uint64_t total_bits = (seg_off[first + nseg - 1] - base) + p.seg_bits[first + nseg - 1];
  const uint64_t total_bytes = (total_bits + 7) >> 3;
  const bool last = k + 1 == nseg;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(p.scratch + (size_t)(u - b - 1) * p.slot_bytes);
  const uint32_t* nxt = last ? nullptr : reinterpret_cast<const uint32_t*>(p.scratch + (size_t)(u - b) * p.slot_bytes);
  const uint64_t o_n = o_k + L_k;  // next segment's offset
  uint8_t* out8 = p.out + p.out_off[b];
  uint32_t* out32 = reinterpret_cast<uint32_t*>(out8);
  auto put = [&](uint32_t w, uint32_t v) {
    if (4ull * w + 4 <= total_bytes) {
      out32[w] = v;
    } else {
      for (uint32_t c = 0; 4ull * w + c < total_bytes; ++c) out8[4ull * w + c] = (uint8_t)(v >> (8 * c));
    }
  };
  // words whose first bit lies in this segment, four per thread (one 16-byte
  // store for a group inside the segment and the stream): word w holds
  // segment bits [32 (w - w_begin) + sh0, + 32), i.e. a funnel shift of
  // slot words w - w_begin and w - w_begin + 1 by the segment's constant sh0
  const uint32_t w_begin = (uint32_t)((o_k + 31) >> 5), w_end = (uint32_t)((o_n + 31) >> 5);
  const uint32_t sh0 = (uint32_t)(32ull * w_begin - o_k);
  const uint32_t nsrc = (L_k + 31) >> 5;  // (the slot's last word is zero-padded past L_k)
  const uint32_t first_next = last ? 0u : nxt[0];  // (the next segment is >= 1024 bits)
  for (uint32_t g = (w_begin >> 2) + threadIdx.x; g < (w_end + 3) >> 2; g += blockDim.x) {
    const int64_t i0 = 4 * (int64_t)g - w_begin;  // slot word of output word 4 g
    uint32_t sw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) sw[j] = i0 + j >= 0 && i0 + j < (int64_t)nsrc ? src[i0 + j] : 0u;
    uint32_t v[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t w = 4 * g + j;
      v[j] = __builtin_amdgcn_alignbit(sw[j + 1], sw[j], sh0);
      if (!last && 32ull * w + 32 > o_n && 32ull * w < o_n) v[j] |= first_next << (uint32_t)(o_n - 32ull * w);
    }
    if (4 * g >= w_begin && 4 * g + 4 <= w_end && 16ull * g + 16 <= total_bytes) {
      *reinterpret_cast<uint4*>(out32 + 4 * (size_t)g) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
        if (4 * g + j >= w_begin && 4 * g + j < w_end) put(4 * g + j, v[j]);
    }
  }
  // the word holding o_1: segment 0's bits below it, segment 1's above
  if (k == 1 && (o_k & 31u) && threadIdx.x == 0) {
    const uint32_t w = (uint32_t)(o_k >> 5), sh = (uint32_t)(o_k & 31u);
    const uint32_t have = 4ull * w < total_bytes ? (uint32_t)min((uint64_t)4, total_bytes - 4ull * w) : 0u;
    uint32_t old = 0;
    for (uint32_t c = 0; c < 4; ++c)
      if (8 * c < sh) old |= (uint32_t)out8[4 * w + c] << (8 * c);
    old &= (1u << sh) - 1u;
    uint32_t v = old | (src[0] << sh);
    if (nseg == 2 && o_n < 32ull * w + 32 && L_k < 32 - sh) v &= (1u << (sh + L_k)) - 1u;
    for (uint32_t c = 0; c < have; ++c) out8[4 * w + c] = (uint8_t)(v >> (8 * c));
  }
  if (last && threadIdx.x == 0) {
    p.out_bytes[b] = total_bytes;
    p.status[b] = RPP_OK;
  }
}

// Host-side kernel choice: SPL 16 for bs > 64 (8 sub-blocks of 128 per
// iteration), else 8; G = next pow2 of ceil(bs / SPL).
typedef void (*EncKernel)(EncParams);
template <uint32_t CS, bool SH>
EncKernel enc_kernel_for(uint32_t bs) {
  if (bs > 64) {
    const uint32_t m = (bs + 15) / 16;
    if (m <= 8) return rpp_encode_kernel<16, 8, CS, SH>;
    if (m <= 16) return rpp_encode_kernel<16, 16, CS, SH>;
    return rpp_encode_kernel<16, 32, CS, SH>;
  }
  const uint32_t m = (bs + 7) / 8;
  if (m <= 1) return rpp_encode_kernel<8, 1, CS, SH>;
  if (m <= 2) return rpp_encode_kernel<8, 2, CS, SH>;
  if (m <= 4) return rpp_encode_kernel<8, 4, CS, SH>;
  return rpp_encode_kernel<8, 8, CS, SH>;
}

// chunks per unit for a batch of total_samples: kEncSegChunks when that gives
// kEncTargetUnits units, else the power of two that comes closest from below
// (a batch of 16 x 64 KiB blocks: 16-chunk units, 16 waves per block)
uint32_t enc_seg_chunks(const rpp_config* cfg, uint64_t total_samples) {
  const uint64_t chunks = total_samples / ((uint64_t)cfg->block_size * cfg->component_stream_count);
  uint32_t c = kEncSegChunks;
  while (c > kEncSegChunksMin && chunks / c < kEncTargetUnits) c >>= 1;
  return c;
}

// streams of more than seg_chunks chunks are split
bool enc_segmented(const rpp_config* cfg, uint64_t total_samples, uint64_t max_stream_samples) {
  return max_stream_samples >
         (uint64_t)enc_seg_chunks(cfg, total_samples) * cfg->block_size * cfg->component_stream_count;
}

EncKernel enc_kernel(const rpp_config* cfg) {
  const bool sh = cfg->unused_lsb_count != 0;
  return cfg->component_stream_count == 1
             ? (sh ? enc_kernel_for<1, true>(cfg->block_size) : enc_kernel_for<1, false>(cfg->block_size))
             : (sh ? enc_kernel_for<2, true>(cfg->block_size) : enc_kernel_for<2, false>(cfg->block_size));
}

// rpp_encode_batch_ws workspace: unit counts and bases, the unit -> stream
// map, per-unit bit counts and offsets, and one worst-case scratch slot per
// segment after a stream's first
struct EncWorkspace {
  uint64_t* units;     // [B + 1]
  uint64_t* seg_base;  // [B + 1]
  uint32_t* seg_map;   // [max_units]
  uint64_t* seg_bits;  // [max_units]
  uint64_t* seg_off;   // [max_units]
  uint8_t* scratch;    // [(max_units - B) * slot_bytes]
  uint64_t slot_bytes, max_units, bytes;
  uint32_t seg_chunks;
};

EncWorkspace enc_layout(const rpp_config* cfg, uint64_t total_samples, uint32_t nblocks, uint8_t* base) {
  const uint64_t B = nblocks;
  EncWorkspace w{};
  w.seg_chunks = enc_seg_chunks(cfg, total_samples);
  const uint64_t seg_samples = (uint64_t)w.seg_chunks * cfg->block_size * cfg->component_stream_count;
  w.max_units = B + total_samples / seg_samples;
  w.slot_bytes = (rpp_worst_case_bytes(cfg, seg_samples) + 16 + 15) & ~uint64_t{15};
  uint64_t off = 0;
  auto take = [&](uint64_t bytes) {
    uint8_t* q = base ? base + off : nullptr;
    off = (off + bytes + 255) & ~uint64_t{255};
    return q;
  };
  w.units = reinterpret_cast<uint64_t*>(take((B + 1) * 8));
  w.seg_base = reinterpret_cast<uint64_t*>(take((B + 1) * 8));
  w.seg_map = reinterpret_cast<uint32_t*>(take(w.max_units * 4));
  w.seg_bits = reinterpret_cast<uint64_t*>(take(w.max_units * 8));
  w.seg_off = reinterpret_cast<uint64_t*>(take(w.max_units * 8));
  w.scratch = take((w.max_units - B) * w.slot_bytes);
  w.bytes = off;
  return w;
}

}  // namespace

extern "C" {

#ifdef RPP_STATS
// Diagnostic build only: copies (and optionally clears) the encode kernel's loop counters.
int rpp_enc_stats_fetch(uint64_t* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_enc_stats), sizeof(uint64_t) * 16) != hipSuccess) return RPP_HIP_ERROR;
  if (reset) {
    uint64_t z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_enc_stats), z, sizeof z) != hipSuccess) return RPP_HIP_ERROR;
  }
  return RPP_OK;
}
#endif

int rpp_encode_batch(const rpp_config* cfg, const uint16_t* d_in, const uint64_t* d_in_offsets,
                     const uint64_t* d_n_samples, uint32_t nblocks, uint8_t* d_out,
                     const uint64_t* d_out_offsets, uint64_t* d_out_bytes, int32_t* d_status,
                     void* stream) {
  int st = rpp_check_config(cfg);
  if (st != RPP_OK) return st;
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_n_samples || !d_out || !d_out_offsets || !d_out_bytes || !d_status)
    return RPP_INVALID_ARGUMENT;
  EncParams p{d_in, d_in_offsets, d_n_samples, d_out, d_out_offsets, d_out_bytes, d_status, nblocks,
              cfg->block_size, cfg->component_stream_count, cfg->big_endian ? 1u : 0u,
              cfg->unused_lsb_count, nullptr, nullptr, nullptr, nullptr, 0, 0, kEncSegChunks};
  hipLaunchKernelGGL(enc_kernel(cfg), dim3(nblocks), dim3(kWave), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

uint64_t rpp_encode_workspace_bytes(const rpp_config* cfg, uint64_t total_samples, uint64_t max_stream_samples,
                                    uint32_t nblocks) {
  if (rpp_check_config(cfg) != RPP_OK) return 0;
  if (!enc_segmented(cfg, total_samples, max_stream_samples)) return 0;
  return enc_layout(cfg, total_samples, nblocks, nullptr).bytes;
}

int rpp_encode_batch_ws(const rpp_config* cfg, const uint16_t* d_in, const uint64_t* d_in_offsets,
                        const uint64_t* d_n_samples, uint32_t nblocks, uint8_t* d_out, const uint64_t* d_out_offsets,
                        uint64_t* d_out_bytes, int32_t* d_status, uint64_t total_samples,
                        uint64_t max_stream_samples, void* d_workspace, uint64_t workspace_bytes, void* stream) {
  int st = rpp_check_config(cfg);
  if (st != RPP_OK) return st;
  if (nblocks == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_n_samples || !d_out || !d_out_offsets || !d_out_bytes || !d_status)
    return RPP_INVALID_ARGUMENT;
  if (!enc_segmented(cfg, total_samples, max_stream_samples))  // no stream to split: one wave per stream
    return rpp_encode_batch(cfg, d_in, d_in_offsets, d_n_samples, nblocks, d_out, d_out_offsets, d_out_bytes,
                            d_status, stream);
  const EncWorkspace w = enc_layout(cfg, total_samples, nblocks, static_cast<uint8_t*>(d_workspace));
  if (!d_workspace || workspace_bytes < w.bytes) return RPP_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t chunk_len = cfg->block_size * cfg->component_stream_count;
  hipLaunchKernelGGL(rpp_enc_units_kernel, dim3((nblocks + 256) / 256), dim3(256), 0, s, d_n_samples, nblocks,
                     chunk_len, w.seg_chunks, w.units);
  if ((st = rpp_exclusive_scan_u64(w.units, (uint64_t)nblocks + 1, w.seg_base, s)) != RPP_OK) return st;
  hipLaunchKernelGGL(rpp_enc_unit_map_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, s, w.seg_base, nblocks,
                     w.max_units, w.seg_map);
  EncParams p{d_in, d_in_offsets, d_n_samples, d_out, d_out_offsets, d_out_bytes, d_status, nblocks,
              cfg->block_size, cfg->component_stream_count, cfg->big_endian ? 1u : 0u,
              cfg->unused_lsb_count, w.seg_map, w.seg_base, w.seg_bits, w.scratch, w.slot_bytes, w.max_units,
              w.seg_chunks};
  hipLaunchKernelGGL(enc_kernel(cfg), dim3((uint32_t)w.max_units), dim3(kWave), 0, s, p);
  if (w.max_units > nblocks) {  // streams long enough to be split: place the segments
    if ((st = rpp_exclusive_scan_u64(w.seg_bits, w.max_units, w.seg_off, s)) != RPP_OK) return st;
    hipLaunchKernelGGL(rpp_enc_concat_kernel, dim3((uint32_t)w.max_units), dim3(256), 0, s, p,
                       (const uint64_t*)w.seg_off);
  }
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}

}  // extern "C"
